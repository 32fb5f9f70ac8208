"""ODE driver for unconditional / class-conditional sampling (reference: flow_matching.py:15-180).

``CNF(net)`` exposes the reference's sampling entry points -- ``decode`` (noise -> data, t: 0 -> 1),
``encode`` (data -> noise, t: 1 -> 0), ``decode_fixadp`` (fixed steps up to t_edit, adaptive after)
-- over this package's own integrators (uspace_amd/odeint.py), because the reference's solver is
the external torchdiffeq.  ``sample_ode`` (the name BASELINE.json uses) aliases ``decode``.

Every keyword reaches the network at each evaluation, classifier-free guidance among them:
``decode(z, y, cfg_scale=s)`` (optionally ``empty_label=K``) integrates v_c + s (v_c - v_u), with
``cfg_scale`` a number or B per-sample values (libs/uvit.py of this package).
"""
import torch
import torch.nn as nn

from .odeint import ADAPTIVE, FIXED, Stats, odeint

_RTOL = 1e-5
_ATOL = 1e-5


class CNFBase(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.last_stats = None        # odeint.Stats of the most recent solve (NFE etc.)
        self.state_ops_factory = None  # None -> odeint.HipStateOps (the only implementation shipped)
        # adaptive step control over a batch sharded across ranks: None = every rank controls its own steps
        # (the reference's behaviour under `accelerate launch`); a process group, or True for the default group = one
        # all-reduced error norm per step attempt, i.e. the step sequence of the unsharded solve on every rank
        self.norm_group = None

    # ------------------------------------------------------------------ reference surface
    def is_dissection_mode(self, kwargs):
        return "dissect_name" in kwargs and kwargs["dissect_name"] is not None

    def get_ode_kwargs(self, **kwargs):
        """Same selection rule and dict shape as the reference (flow_matching.py:38-85)."""
        if not self.is_dissection_mode(kwargs):
            return dict(method="dopri5", rtol=_RTOL, atol=_ATOL, adjoint_params=())
        sk = kwargs["solver_kwargs"]
        fixed = dict(method=sk.get("solver_fix"), rtol=_RTOL, atol=_ATOL, adjoint_params=(),
                     options=dict(step_size=sk.get("solver_fix_step")))
        adaptive = dict(method=sk.get("solver_adaptive"), rtol=_RTOL, atol=_ATOL, adjoint_params=())
        if sk["solver"] == "fixed":
            return fixed
        if sk["solver"] == "adaptive":
            return adaptive
        if sk["solver"] == "fixadp":
            return fixed, adaptive
        raise NotImplementedError(f"solver={sk['solver']}")

    def training_losses(self, *args, **kwargs):
        raise NotImplementedError(
            "uspace_amd implements the sampling hot path only (forward kernels, no backward); "
            "train with the reference's PyTorch modules and load the state_dict here")

    # ------------------------------------------------------------------ integration helpers
    def _velocity(self, t, x, cond, kwargs):
        raise NotImplementedError

    def forward(self, t, x, *cond_args, **kwargs):
        raise NotImplementedError

    def _timesteps(self, t, x):
        """(B,) stride-0 fp32 view of the scalar time, like ``t.expand(B)`` (flow_matching.py:33).

        READ-ONLY: on a fixed time grid (``_grid_is_fixed``, set by ``_integrate`` for the duration of its solve from the solver method / ``n_steps``) the
        device scalar behind the view is cached per (device, t) and handed out again in every later evaluation and solve -- a
        fixed-step solve visits the same times every time, and the cache saves one fill launch per evaluation.  A consumer
        that wrote into it (``t *= 1000`` in a ``_velocity`` override or a hook) would change that time for every later use;
        the reference's own ``t.expand(B)`` view has the same aliasing.  Error-controlled solves choose their own times, no
        two alike: they get a fresh scalar per call and never touch the cache, which is bounded (oldest entry out first)."""
        if torch.is_tensor(t):
            if t.numel() != 1:
                return t, None
            th = float(t.item())
        else:
            th = float(t)
        if not getattr(self, "_grid_is_fixed", False):
            return torch.full((), th, dtype=torch.float32, device=x.device).expand(x.shape[0]), th
        cache = self.__dict__.setdefault("_t_scalars", {})
        key = (x.device, th)
        ts = cache.get(key)
        if ts is None:
            while len(cache) >= self._T_SCALARS_MAX:
                cache.pop(next(iter(cache)))
            ts = cache[key] = torch.full((), th, dtype=torch.float32, device=x.device)
        return ts.expand(x.shape[0]), th

    _T_SCALARS_MAX = 512

    def _integrate(self, func, y0, t0, t1, ode_kwargs, n_steps=None):
        stats = self.last_stats if self.last_stats is not None else Stats()
        opts = ode_kwargs.get("options") or {}
        if self.state_ops_factory is not None:
            ops = self.state_ops_factory(y0)
        elif self.norm_group is not None:
            from .odeint import HipStateOps
            ops = HipStateOps(y0, group=self.norm_group)
        else:
            ops = None
        # fixed grid (euler / midpoint / rk4, or an error-controlled method run on n_steps equal steps): the times repeat.  The flag
        # holds for THIS solve only: a forward() / _velocity() call outside a solve (or a solve nested in a hook) gets fresh scalars
        prev = getattr(self, "_grid_is_fixed", False)
        self._grid_is_fixed = ode_kwargs["method"] in FIXED or n_steps is not None
        try:
            out = odeint(func, y0, float(t0), float(t1), method=ode_kwargs["method"], rtol=ode_kwargs["rtol"],
                         atol=ode_kwargs["atol"], step_size=opts.get("step_size"), n_steps=n_steps, stats=stats, ops=ops)
        finally:
            self._grid_is_fixed = prev
        self.last_stats = stats
        return out

    def _solve(self, cond, x, t0, t1, kwargs, force_fixed=False, func=None):
        self.last_stats = Stats()
        if func is None:
            func = lambda t, xx: self._velocity(t, xx, cond, kwargs)
        sk = kwargs["solver_kwargs"]            # KeyError if absent, as in the reference
        n_steps = sk.get("n_steps") if hasattr(sk, "get") else None
        if force_fixed:
            okw = dict(method=sk["solver_fix"], rtol=_RTOL, atol=_ATOL, adjoint_params=(),
                       options=dict(step_size=sk["solver_fix_step"]))
            return self._integrate(func, x, t0, t1, okw, n_steps)
        if sk["solver"] in ("fixed", "adaptive"):
            return self._integrate(func, x, t0, t1, self.get_ode_kwargs(**kwargs), n_steps)
        if sk["solver"] == "fixadp":
            return self._fixadp(func, x, t0, kwargs["t_edit"], t1, kwargs)
        raise NotImplementedError(f"unknown solver {sk}")

    def _fixadp(self, func, z, t0, t_mid, t1, kwargs):
        assert 0 <= t_mid <= 1, f"t_mid={t_mid}"
        fixed_kw, adaptive_kw = self.get_ode_kwargs(**kwargs)
        mid = self._integrate(func, z, t0, t_mid, fixed_kw)
        return self._integrate(func, mid, t_mid, t1, adaptive_kw)

    # ------------------------------------------------------------------ local edits: the paired solve
    _WRITE_NAMES = ("write_attr", "write_pca")

    def _local_kwargs(self, B, kwargs):
        """The keywords of a paired solve over 2B rows (source rows first) from those of the edit: the refusals, ``write_scale`` as
        ``cat(zeros(B), s)`` and ``target_context_ids`` as ``[empty] * B + ids`` -- the per-row mechanisms the network already has.
        Host work only."""
        import numpy as np
        if kwargs.get("cfg_scale") is not None:
            raise ValueError("decode_local under cfg_scale is not supported: a guided local edit would run 4B rows")
        if kwargs.get("dissect_name") == "read":
            raise ValueError("decode_local with a read hook is not supported: the hook would save the 2B rows of both branches")
        if kwargs.get("vis_am_path") is not None:
            raise ValueError("decode_local with vis_am_path is not supported: draw the maps in a plain decode")
        kw = dict(kwargs)
        if kw.get("dissect_name") in self._WRITE_NAMES:
            s = kw.get("write_scale")
            if torch.is_tensor(s):
                s = s.detach().cpu().numpy()
            s = np.asarray(0.0 if s is None else s, dtype=np.float32).reshape(-1)
            if s.size not in (1, B):
                raise ValueError(f"write_scale has {s.size} entries for a batch of {B}")
            kw["write_scale"] = np.concatenate([np.zeros(B, np.float32), np.broadcast_to(s, (B,))])
        if kw.get("target_context_ids") is not None:
            ids = list(kw["target_context_ids"])
            if len(ids) != B:
                raise ValueError(f"target_context_ids holds {len(ids)} lists for a batch of {B}")
            kw["target_context_ids"] = [np.array([], dtype=np.int64) for _ in range(B)] + ids
        return kw

    def _local_mask(self, mask, z):
        """``mask`` of ``decode_local`` -> a contiguous fp32 device tensor [B, S * S], or the mask object itself where it is made at
        every evaluation (``tools.local_edit.AttentionWordMask``)."""
        import numpy as np
        from .tools import local_edit
        B, S = z.shape[0], z.shape[-1]
        if isinstance(mask, local_edit.AttentionWordMask):
            return mask
        if isinstance(mask, local_edit.LabelRegionMask):
            if mask.mask is None:
                raise ValueError("the LabelRegionMask is not bound to images: pass region.of(images, S)")
            mask = mask.mask
        if mask is None:
            raise ValueError("decode_local needs mask=")
        m = mask.detach() if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask, dtype=np.float32)))
        shape = tuple(m.shape)
        if z.dim() != 4 or z.shape[2] != S or shape not in ((S, S), (B, S, S), (B, 1, S, S)):
            raise ValueError(f"mask must be [{S},{S}], [{B},{S},{S}] or [{B},1,{S},{S}] for latents {tuple(z.shape)}, got {shape}")
        m = m.to(torch.float32)
        if not bool(((m >= 0) & (m <= 1)).all()):            # NaN compares false
            raise ValueError("mask values must lie in [0, 1] (and none may be NaN)")
        if m.dim() == 2:
            m = m.expand(B, S, S)
        return m.to(z.device).reshape(B, S * S).contiguous()

    def _decode_local(self, z, cond2, mask, kwargs, maps_velocity=None):
        """The paired solve: state of 2B rows (source rows first, both branches from ``z``), one network call over the 2B rows per
        evaluation (always eager), then one ``uspace_pair_blend`` that puts the source's velocity in the edited rows wherever the
        mask is 0.  Goes through ``_solve`` like every decode; ``last_stats`` counts evaluations of 2B rows, and an error-controlled
        solve takes its norm over the 2B rows.  -> (edited, source)."""
        from . import _hip
        B = z.shape[0]
        kw = self._local_kwargs(B, kwargs)
        m = self._local_mask(mask, z)
        z2 = torch.cat([z, z])

        def blended(v, mm):
            if v.dtype == torch.float32 and v.is_contiguous():
                return _hip.pair_blend(v, mm)
            return _hip.pair_blend(v.to(torch.float32).contiguous(), mm).to(v.dtype)

        if torch.is_tensor(m):
            func = lambda t, xx: blended(self._velocity(t, xx, cond2, kw), m)
        else:
            if maps_velocity is None:
                raise ValueError("an AttentionWordMask needs the text-to-image driver: this network has no word columns")
            m.check(self.net, B)

            def func(t, xx):
                _ts, th = self._timesteps(t, xx)
                if th is None:
                    raise ValueError("an AttentionWordMask needs one time for the whole batch")
                if m.all_ones_at(th):
                    return self._velocity(t, xx, cond2, kw)             # mask == 1: the edited rows keep their own velocity
                v, maps = maps_velocity(t, xx, cond2, kw, m.window(self.net))
                return blended(v, m.from_maps(self.net, maps, th))

        out = self._solve(cond2, z2, 0.0, 1.0, kw, func=func)
        return out[B:], out[:B]


class CNF(CNFBase):
    """``CNF(net).decode(z, y, **kwargs)``; the net is called as ``net(x, t, y, **kwargs)``."""

    def forward(self, t, x, y=None, **kwargs):
        ts, th = self._timesteps(t, x)
        if th is not None and "_t_host" not in kwargs:
            kwargs = dict(kwargs, _t_host=th)
        pred, _aux = self.net(x, ts, y, **kwargs)            # nnet returns (pred, None), flow_matching.py:34
        return pred

    def _velocity(self, t, x, cond, kwargs):
        return self.forward(t, x, cond, **kwargs)

    def encode(self, x, y=None, **kwargs):
        """Data -> noise with the FIXED solver, t: 1 -> 0 (flow_matching.py:102-128)."""
        return self._solve(y, x, 1.0, 0.0, kwargs, force_fixed=True)

    def decode(self, z, y=None, **kwargs):
        """Noise -> data, t: 0 -> 1 (flow_matching.py:130-151)."""
        return self._solve(y, z, 0.0, 1.0, kwargs)

    def decode_fixadp(self, z, y, t_mid, **kwargs):
        self.last_stats = Stats()
        func = lambda t, xx: self._velocity(t, xx, y, kwargs)
        return self._fixadp(func, z, 0.0, t_mid, 1.0, kwargs)

    sample_ode = decode

    def decode_local(self, z, y=None, *, mask=None, source=None, **kwargs):
        """A local edit: ``decode(z, y, **kwargs)`` (a ``write_attr`` / ``write_pca`` edit) and the same decode without the edit in
        one paired solve, the edited branch following the source's velocity wherever ``mask`` is 0 -> (edited, source).  Outside the
        mask the edited latents are bit-equal to the source's under every solver.  ``mask``: [S, S], [B, S, S] or [B, 1, S, S] in
        [0, 1], or a ``tools.local_edit.LabelRegionMask`` bound to images.  ``source``: ``dict(y=...)``, the source branch's labels
        where they differ."""
        ys = (source or {}).get("y", y)
        if (y is None) != (ys is None):
            raise ValueError("y and source['y'] must both be given or both be None")
        y2 = None
        if y is not None:
            y = torch.as_tensor(y).reshape(-1)
            y2 = torch.cat([torch.as_tensor(ys).reshape(-1).to(y.device), y])
        return self._decode_local(z, y2, mask, kwargs)

    def decode_write_scales(self, z, y, write_scales, **kwargs):
        """The reference's sweep ``for write_scale in write_scales: decode(z, write_scale=...)``
        (tools/utils_vis.py:189-198, one full solve of the same z per scale).  Returns [n_scales, B, C, H, W].

        A fixed-step solve runs as ONE solve over len(scales)*B rows with a per-row hook scale: the rows never
        interact, so it equals the sequential sweep.  An error-controlled solve picks its steps from one norm over
        all its rows, so it is split where the reference's solves differ: ``fixadp`` runs its fixed leg batched
        and then one adaptive leg per scale over that scale's B rows; ``adaptive`` runs one solve per scale.
        ``last_stats`` sums the NFE / attempts of every solve."""
        n, B = len(write_scales), z.shape[0]
        scales = [float(s) for s in write_scales]
        rows = torch.as_tensor(scales, dtype=torch.float32).repeat_interleave(B)
        zz = z.repeat(n, 1, 1, 1)
        yy = y.repeat(n) if torch.is_tensor(y) else y
        split = self._error_controlled_legs(kwargs)
        if split is None:
            out = self.decode(zz, yy, **dict(kwargs, write_scale=rows))
            return out.view(n, B, *z.shape[1:])
        stats = Stats()
        if split == "adaptive":
            outs = []
            for s in scales:
                outs.append(self.decode(z, y, **dict(kwargs, write_scale=s)))
                _add_stats(stats, self.last_stats)
        else:                                   # fixadp: batched fixed leg to t_edit, then one adaptive leg per scale
            t_mid = kwargs["t_edit"]
            assert 0 <= t_mid <= 1, f"t_mid={t_mid}"
            fixed_kw, adaptive_kw = self.get_ode_kwargs(**kwargs)
            kw_rows = dict(kwargs, write_scale=rows)
            self.last_stats = stats
            mid = self._integrate(lambda t, xx: self._velocity(t, xx, yy, kw_rows), zz, 0.0, t_mid, fixed_kw)
            outs = []
            for i, s in enumerate(scales):
                kw_i = dict(kwargs, write_scale=s)
                self.last_stats = stats
                outs.append(self._integrate(lambda t, xx, kw_i=kw_i: self._velocity(t, xx, y, kw_i), mid[i * B:(i + 1) * B],
                                            t_mid, 1.0, adaptive_kw))
        self.last_stats = stats
        return torch.stack(outs)

    def _error_controlled_legs(self, kwargs):
        """Which legs of decode(**kwargs) are error-controlled: None (none: fixed steps), "adaptive" (the whole solve) or
        "fixadp" (the leg after t_edit).  Follows _solve's selection."""
        sk = kwargs["solver_kwargs"]
        n_steps = sk.get("n_steps") if hasattr(sk, "get") else None
        if sk["solver"] in ("fixed", "adaptive"):
            okw = self.get_ode_kwargs(**kwargs)
            return "adaptive" if okw["method"] in ADAPTIVE and n_steps is None else None
        if sk["solver"] == "fixadp":
            return "fixadp" if self.get_ode_kwargs(**kwargs)[1]["method"] in ADAPTIVE else None
        return None


def _add_stats(total, part):
    total.nfe += part.nfe
    total.accepted += part.accepted
    total.rejected += part.rejected
