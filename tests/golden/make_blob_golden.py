#!/usr/bin/env python3
"""Records what the library reports and writes for the packed weight blobs (tests/blob_cases.py says for which models):

  blob_sizes.json     num_params, every param_numel(i), weight_bytes and workspace_bytes at B = 1, 3, 8, 64 of every pinned
                      configuration -- host queries, no GPU needed.                            (``make_blob_golden.py sizes``)
  blob_digests.json   sha256 of the blob ``uspace_*_pack_weights`` writes into zeroed memory for each tiny model, packed
                      twice and required to agree -- needs the GPU.                            (``make_blob_golden.py digests``)

Run at the commit whose layout is to be pinned; the commit is written into both files.  Reads nothing outside the repository."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import blob_cases as C  # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("USPACE_GOLDEN_COMMIT", "unknown")


def write(name, payload, out_dir):
    path = os.path.join(out_dir, name)
    with open(path, "w") as f:
        json.dump(payload, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    if what == "sizes":
        write("blob_sizes.json", dict(recorded_at_commit=commit(), sizes=C.size_table(HERE)), out_dir)
    elif what == "digests":
        digests = {}
        for kind in C.TINY_KINDS:
            _m, prefix, cfg, tensors = C.tiny_model(kind, HERE)
            first, second = C.blob_digest(prefix, cfg, tensors), C.blob_digest(prefix, cfg, tensors)
            assert first == second, f"{kind}: two packs of the same weights differ"
            digests[kind] = first
            print(kind, first)
        write("blob_digests.json", dict(recorded_at_commit=commit(), packed_twice_equal=True, digests=digests), out_dir)
    else:
        raise SystemExit("usage: make_blob_golden.py sizes|digests [output directory]")


if __name__ == "__main__":
    main()
