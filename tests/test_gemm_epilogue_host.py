"""Two epilogue forms of the 256 x 256 GEMM bodies that were built, measured and not landed (profiles/epilogue_forms.md; kept as
tools/lab/dropped/gemm_full_line_f32_role_bodies.patch and gemm_early_epilogue_last_ktile.patch), on the host: NumPy models of what
each must preserve, so that whoever takes one up again starts from a checked statement of it.

Whole-line fp32 stores.  In the epilogue the lane (fr = lane % 16, fq = lane / 16) of a wave holds, for row sub-tile i and column
sub-tile j, the four values of row 16 i + fr, columns 16 j + 4 fq .. + 3.  The product stores sub-tile j with one instruction: 16 rows
x 64 bytes.  The dropped form takes the sub-tiles in pairs (j, j + 1), swaps the two halves of every 16-lane group between them with
DPP row_ror:8 under bank masks, and stores rows 0-7 with all 128 bytes in one instruction and rows 8-15 in the next.  The model tags
every value with its (row, column) and shows that the exchange is a permutation that sends every value to its own address, that each
instruction writes 8 whole 128-byte lines, and that nothing is written outside the wave's 16 x 64 block.

Epilogue under the last K tile.  The product's last K tile runs its MFMAs phase by phase (k-slice 0 of both row-halves, then k-slice
1); the dropped form gives row sub-tile i all 2 TN of its MFMAs together, in ascending i.  An fp32 accumulator's bits depend on the
order in which IT receives its K slices and on nothing else, so the model lists both orders and shows that every accumulator sees
k-slice 0 before k-slice 1 in both, each exactly once."""
import numpy as np
import pytest

WAVE, TN = 64, 4          # lanes; 16-column sub-tiles per wave in the 256 x 256 form (BN / WN / 16)


def update_dpp_row_ror8(old, src, bank_mask):
    """v_mov_b32_dpp row_ror:8 row_mask:0xf bank_mask:<bank_mask>, bound_ctrl off: lane l of a 16-lane row reads lane (l - 8) mod 16 of
    the same row; lanes whose bank (4 lanes) is masked off keep ``old``."""
    lane = np.arange(WAVE)
    from_lane = (lane & ~15) | ((lane - 8) & 15)
    enabled = (bank_mask >> ((lane & 15) >> 2)) & 1
    return np.where(enabled[:, None].astype(bool), src[from_lane], old)


def line_pair(l, r):
    """line_pair of the dropped patch on [lane, 4] arrays."""
    return update_dpp_row_ror8(l, r, 0xC), update_dpp_row_ror8(r, l, 0x3)


def wave_values(ld):
    """tag[j][lane, c]: the element offset row * ld + column (inside the wave's block) of the value the lane holds for sub-tile j."""
    lane = np.arange(WAVE)
    fr, fq = lane & 15, lane >> 4
    return [fr[:, None] * ld + 16 * j + 4 * fq[:, None] + np.arange(4)[None, :] for j in range(TN)]


@pytest.mark.parametrize("ld", (64, 1024, 1028, 4100))
def test_full_line_exchange_sends_every_value_to_its_own_address(ld):
    lane = np.arange(WAVE)
    fr, fq = lane & 15, lane >> 4
    v = wave_values(ld)
    written = {}
    # the kernel: po = row (fr & 7), column 16 (fr >> 3) + 4 fq; per pair j: lo at po + 16 j, hi at po + 16 j + 8 ld
    po = (fr & 7) * ld + 16 * (fr >> 3) + 4 * fq
    for j in range(0, TN, 2):
        lo, hi = line_pair(v[j], v[j + 1])
        for data, base in ((lo, po + 16 * j), (hi, po + 16 * j + 8 * ld)):
            addr = base[:, None] + np.arange(4)[None, :]
            assert np.array_equal(addr, data), "a value leaves for an address that is not its own"
            # one instruction: 8 rows, each a whole aligned run of 32 floats (128 bytes)
            rows = np.unique(addr // ld)
            assert len(rows) == 8
            for row in rows:
                cols = np.sort(addr[addr // ld == row] % ld)
                assert np.array_equal(cols, np.arange(32) + 16 * j) and (16 * j) % 32 == 0
            for a in addr.ravel():
                assert a not in written, "an address is written twice"
                written[a] = True
    # a permutation of the wave's 16 rows x 64 columns: every element once, nothing else
    want = (np.arange(16)[:, None] * ld + np.arange(16 * TN)[None, :]).ravel()
    assert np.array_equal(np.sort(np.fromiter(written, np.int64)), np.sort(want))


def test_exchange_is_a_permutation_of_the_lanes_values():
    v = wave_values(64)
    lo, hi = line_pair(v[0], v[1])
    assert np.array_equal(np.sort(np.concatenate([lo, hi]).ravel()), np.sort(np.concatenate([v[0], v[1]]).ravel()))
    # lanes 0-7 of a group keep their left half in lo, lanes 8-15 their right half in hi: half of the values do not move
    lane = np.arange(WAVE)
    assert np.array_equal(lo[(lane & 15) < 8], v[0][(lane & 15) < 8]) and np.array_equal(hi[(lane & 15) >= 8], v[1][(lane & 15) >= 8])


def test_a_wrong_bank_mask_is_seen():
    """The model is not vacuous: with the two bank masks exchanged, values leave for other addresses."""
    v = wave_values(64)
    lo = update_dpp_row_ror8(v[0], v[1], 0x3)
    lane = np.arange(WAVE)
    po = ((lane & 15) & 7) * 64 + 16 * ((lane & 15) >> 3) + 4 * (lane >> 4)
    assert not np.array_equal(po[:, None] + np.arange(4)[None, :], lo)


HM, TM = 4, 8           # row sub-tiles per row-half and per wave in the 256 x 256 form


def product_last_tile_order():
    """(i, j, k-slice) of the MFMAs of KTILE in gemm.hip, in issue order: the MMA(af, wf, mh, ilo, ihi) calls of the macro, each a snake
    over the column sub-tiles."""
    def mma(ks, mh, ilo, ihi):
        return [(mh * HM + i, (TN - 1 - jj) if i & 1 else jj, ks) for i in range(ilo, ihi) for jj in range(TN)]
    return (mma(0, 0, 0, 1) + mma(0, 0, 1, HM) + mma(0, 1, 0, 1) + mma(0, 1, 1, HM) + mma(1, 0, 0, 1) + mma(1, 0, 1, HM) +
            mma(1, 1, 0, HM // 2) + mma(1, 1, HM // 2, HM))


def early_last_tile_order():
    """... of the dropped form: per row sub-tile, k-slice 0 over the column sub-tiles, then k-slice 1 over them the other way round."""
    order = []
    for i in range(TM):
        order += [(i, (TN - 1 - jj) if i & 1 else jj, 0) for jj in range(TN)]
        order += [(i, jj if i & 1 else (TN - 1 - jj), 1) for jj in range(TN)]
    return order


def k_order_per_accumulator(order):
    seen = {}
    for i, j, ks in order:
        seen.setdefault((i, j), []).append(ks)
    return seen


def test_early_last_tile_keeps_every_accumulators_k_order():
    old, new = k_order_per_accumulator(product_last_tile_order()), k_order_per_accumulator(early_last_tile_order())
    assert sorted(old) == sorted(new) == [(i, j) for i in range(TM) for j in range(TN)]
    assert all(v == [0, 1] for v in old.values()) and old == new
    # and the dropped order is what it claims: all MFMAs of row sub-tile i together, in ascending i
    rows = [i for i, _, _ in early_last_tile_order()]
    assert rows == sorted(rows) and len(rows) == 2 * TM * TN == len(product_last_tile_order())
