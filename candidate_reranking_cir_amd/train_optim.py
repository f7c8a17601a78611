"""`AdamW`: torch.optim.AdamW's update rule on cir_adamw_step for the trainers' flat parameter slabs (train_core._Slab), with GradScaler's
found_inf / skip decision taken on the device, and torch.optim's `state_dict()` / `load_state_dict()` for the reference's checkpoints
(utils.save_model); several parameter groups (own lr / weight_decay / eps / lr_scale) and clip_grad_norm_'s global-norm clip decided on the
device as well (cir_grads_sumsq, cir_adamw_begin_clip, cir_adamw_step_groups); `cosine_lr_schedule`, `warmup_lr_schedule`,
`step_lr_schedule`, `exp_lr_schedule`: the reference's schedules (utils.py:216-241)."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np

import torch
from torch.autograd.graph import increment_version

from . import train_ops as T
from .train_core import _SLABS, _Slab


def cosine_lr_schedule(optimizer, epoch: int, max_epoch: int, init_lr: float, min_lr: float) -> float:
    """utils.cosine_lr_schedule (utils.py:216-221): the per-epoch decay stage2_train.py:159 applies; works on `AdamW` below and on torch.optim."""
    lr = (init_lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * epoch / max_epoch)) + min_lr
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def warmup_lr_schedule(optimizer, step: int, max_step: int, init_lr: float, max_lr: float) -> float:
    """utils.warmup_lr_schedule (utils.py:223-228)."""
    lr = min(max_lr, init_lr + (max_lr - init_lr) * step / max_step)
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def step_lr_schedule(optimizer, epoch: int, init_lr: float, min_lr: float, decay_rate: float) -> float:
    """utils.step_lr_schedule (utils.py:230-235)."""
    lr = max(min_lr, init_lr * (decay_rate ** epoch))
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def exp_lr_schedule(optimizer, epoch: int, gamma: float) -> None:
    """utils.exp_lr_schedule (utils.py:237-241): every group's OWN lr times gamma (`epoch` is not used there either)."""
    for group in optimizer.param_groups:
        group["lr"] *= gamma


class _Work(NamedTuple):
    """One update launch of `AdamW.step`: flat (or per-tensor) parameters, gradients and moments; the 16-bit copy written along and the
    slab it belongs to (flat path); the non-contiguous parameter a stepped copy is written back to (per-tensor path)."""
    p: torch.Tensor
    g: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    p16: Optional[torch.Tensor] = None
    slab: Optional[_Slab] = None
    copy_back: Optional[torch.nn.Parameter] = None
    table: Optional["T.SegmentTable"] = None      # several groups in one flat launch: the cached segment table
    group: int = 0                                # without a table: the group of every element


class AdamW:
    """torch.optim.AdamW's update rule on cir_adamw_step (stage2_train.py:138 builds that optimizer), fp32 master parameters.
    When the parameters and their gradients are the trainer's flat buffers (the normal case after `fusion_train`), one launch
    updates all of them; otherwise one launch per tensor.  `params`: an iterable of parameters or a list of group dicts as torch.optim
    takes them ({"params", and optionally "lr", "weight_decay", "eps", "lr_scale"}; at most 8).  A group's applied rate is
    float32(group["lr"] * group.get("lr_scale", 1.0)): the reference's schedules overwrite "lr" in every group (utils.py:216-241), so the
    ratio between groups lives in its own key (timm's convention).  `max_grad_norm`: torch.nn.utils.clip_grad_norm_ over everything the
    step applies, decided on the device.  One group without lr_scale and without clipping steps exactly as before."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, model=None, check_finite=None, max_grad_norm=None):
        """`model`: the BLIP_NLVR whose parameters these are (its trainers' finite flags decide the skip; every step() moves the
        parameters' version counters, which the packed inference engines and the 16-bit slabs compare, with or without it).
        `check_finite`: test the gradients step() is about to apply for inf / NaN and skip the update then (GradScaler.step's found_inf,
        stage2_train.py:215-218; one reduction over the flat gradient buffer + one host read).  None = automatic: always, unless `model`
        is given and its trainers run bf16 operands (whose pass cannot overflow: no loss scale).  It governs the steps WITHOUT clipping
        only: with `max_grad_norm` the norm pass reads every gradient buffer anyway and sets the same flag, so a clipped step is always
        tested (`check_finite=False` changes nothing there, and a trainer's own earlier test of the buffer is not reused).
        `max_grad_norm`: finite and > 0, or None (no clipping).
        An empty `params` raises ValueError, as torch.optim does (before parameter groups existed an empty list was accepted and step()
        did nothing)."""
        self.model = model
        self.check_finite = check_finite
        params = list(params)
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        if any(isinstance(g, dict) for g in params):
            if not all(isinstance(g, dict) for g in params):
                raise TypeError("AdamW: `params` mixes parameters and group dicts")
            raw = params
        else:
            raw = [{"params": params}]
        if len(raw) > T.MAX_GROUPS:
            raise ValueError(f"AdamW: {len(raw)} parameter groups; cir_adamw_step_groups takes at most {T.MAX_GROUPS}")
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f"AdamW: max_grad_norm must be finite and > 0, not {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        groups, seen = [], set()
        for k, g in enumerate(raw):
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            ps = [p for p in ps if p.requires_grad]
            if any(id(p) in seen for p in ps):
                raise ValueError("some parameters appear in more than one parameter group")
            seen.update(id(p) for p in ps)
            if "betas" in g and tuple(g["betas"]) != tuple(betas):
                raise ValueError(f"AdamW: group {k} has betas {tuple(g['betas'])}, the optimizer {tuple(betas)}: one cir_adamw_begin computes "
                                 "one pair of bias corrections, so the betas are shared")
            group = {"params": ps, "lr": g.get("lr", lr), "betas": betas, "eps": g.get("eps", eps), "weight_decay": g.get("weight_decay", weight_decay)}
            if "lr_scale" in g:
                group["lr_scale"] = g["lr_scale"]
            groups.append(group)
        self.params = groups[0]["params"] if len(groups) == 1 else [p for g in groups for p in g["params"]]
        self.betas, self.eps, self.wd = betas, groups[0]["eps"], groups[0]["weight_decay"]
        self._state = None                                    # device: [found_inf, t, skipped, bc1, bc2, ...] (cir_adamw_begin)
        self._calls = 0
        self._plans: Dict[tuple, tuple] = {}                  # (param storage, first param) -> cached flat layout of a parameter group
        # torch.optim's surface as far as the reference's loop uses it: utils.cosine_lr_schedule (utils.py:216-221, called once per epoch at
        # stage2_train.py:159) writes `param_group['lr']`; one group, its 'lr' is what step() applies
        self.param_groups = groups
        self._tables: Dict[tuple, tuple] = {}                 # plan key -> (group of every parameter, segment table or None, group)
        self._partials = None                                 # float64 workspace of the norm passes of one step
        self.m: Dict[int, torch.Tensor] = {}
        self.v: Dict[int, torch.Tensor] = {}
        self._flats: Dict[int, tuple] = {}                    # param storage ptr -> (m flat, v flat)

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value: float):
        self.param_groups[0]["lr"] = value

    @staticmethod
    def _flat_range(tensors):
        """(base pointer, elements) when `tensors` tile ONE storage completely in slices padded to 8 elements, else None."""
        st = tensors[0].untyped_storage()
        if any(t.untyped_storage().data_ptr() != st.data_ptr() or not t.is_contiguous() for t in tensors):
            return None
        if sum((t.numel() + 7) // 8 * 8 for t in tensors) * 4 != st.nbytes():
            return None
        return st.data_ptr(), st.nbytes() // 4

    # applied / skipped step counts live on the device (the skip decision is taken there): reading them is a host read
    @property
    def t(self) -> int:
        return 0 if self._state is None else int(self._state[1])

    @property
    def skipped_steps(self) -> int:
        return 0 if self._state is None else int(self._state[2])

    # what cir_adamw_begin_clip left of the last clipped step: host reads as well
    @property
    def grad_norm(self) -> float:
        """The global gradient norm of the last step before clipping (fp32; inf / NaN on a skipped step)."""
        return 0.0 if self._state is None else float(self._state[6:7].view(torch.float32))

    @property
    def clip_coef(self) -> float:
        """min(1, max_grad_norm / (grad_norm + 1e-6)) of the last step; 0 on a skipped one."""
        return 1.0 if self._state is None else float(self._state[5:6].view(torch.float32))

    def _grouped(self) -> bool:
        """Whether step() takes the segmented kernels: more than one group, a group with an lr_scale, or clipping."""
        return len(self.param_groups) > 1 or self.max_grad_norm is not None or "lr_scale" in self.param_groups[0]

    def _segments(self, grp, plan, group_of):
        """(segment table or None, group) of a flat storage: one segment per run of parameters of one group, in storage order; a slab of
        ONE group needs no table.  Cached per plan and per assignment of its parameters to groups; the table lives on the device."""
        ids = tuple(group_of[id(p)] for p in grp)
        key = (plan[0], len(grp), id(grp[0]), id(grp[-1]))
        hit = self._tables.get(key)
        if hit is None or hit[0] != ids:
            order = sorted(range(len(grp)), key=lambda j: plan[2][j])
            ends, seg_ids = [], []
            for a, b in zip(order, order[1:] + [None]):
                end = plan[1] if b is None else plan[2][b]
                if seg_ids and seg_ids[-1] == ids[a]:
                    ends[-1] = end
                else:
                    ends.append(end); seg_ids.append(ids[a])
            table = None if len(ends) == 1 else T.SegmentTable(ends, seg_ids, grp[0].device)
            hit = self._tables[key] = (ids, table, seg_ids[0])
        return hit[1], hit[2]

    def _plan(self, grp):
        """Flat layout of a group of parameters that tile ONE fp32 storage (the trainer's slab): (base pointer, elements, per-parameter
        element offsets) - computed once per group; None when they do not tile one."""
        key = (grp[0].data.untyped_storage().data_ptr(), len(grp), id(grp[0]), id(grp[-1]))
        if key not in self._plans:
            fp = self._flat_range([p.data for p in grp])
            self._plans[key] = None if fp is None else (fp[0], fp[1], [(p.data_ptr() - fp[0]) // 4 for p in grp])
        return self._plans[key]

    @staticmethod
    def _grads_match(grp, plan):
        """The gradients of `grp` are slices of ONE flat buffer laid out like the parameters (what the trainers install): its base pointer."""
        g0 = grp[0].grad
        base = g0.data_ptr() - 4 * plan[2][0]
        if g0.untyped_storage().data_ptr() != base or g0.untyped_storage().nbytes() != 4 * plan[1]:
            return None
        for p, o in zip(grp, plan[2]):
            g = p.grad
            if g.data_ptr() != base + 4 * o or g.dtype != torch.float32 or not g.is_contiguous():
                return None
        return base

    @torch.no_grad()
    def step(self):
        """One AdamW step; with fp16 operands the update is skipped when a gradient is inf / NaN (GradScaler.step, stage2_train.py:215-218).
        Nothing here reads the device (round 6): the finite test ORs into a device flag, cir_adamw_begin turns it into the step count /
        bias corrections or the skip count, and the update kernels return at once under a set flag.  The test runs on the buffers this call
        APPLIES - .grad as it is now, after any accumulation over micro-batches - and does not depend on `model=`."""
        ps = [p for p in self.params if p.grad is not None]
        if not ps:
            return
        dev = ps[0].device
        if self._state is None:
            self._state = torch.zeros((8,), dtype=torch.int32, device=dev)
        st = self._state
        self._calls += 1
        st[0:1].zero_()
        need = self.check_finite
        trainers = [] if self.model is None else [tr for tr in (getattr(self.model, "_trainer", None), getattr(self.model, "_vit_trainer", None)) if tr is not None]
        if need is None:
            need = self.model is None or not trainers or any(getattr(tr, "dtype", None) == torch.float16 for tr in trainers)
        for tr in trainers:                                   # a flag a trainer's last backward (or a test / caller) set
            gf = getattr(tr, "grads_finite", None)
            if gf is not None:
                st[0:1] |= (~torch.as_tensor(gf, device=dev).reshape(1)).to(torch.int32)
        # one launch per FLAT STORAGE (the two-branch encoder's slab; the ViT's when it is fine-tuned), per tensor for what is left
        grouped = self._grouped()
        group_of = {id(p): k for k, g in enumerate(self.param_groups) for p in g["params"]} if grouped else None
        groups: Dict[int, list] = {}
        for p in ps:
            groups.setdefault(p.data.untyped_storage().data_ptr(), []).append(p)
        work = []
        for grp in groups.values():
            plan = self._plan(grp) if len(grp) > 1 else None
            gbase = self._grads_match(grp, plan) if plan is not None else None
            if gbase is None:
                for p in grp:
                    if id(p) not in self.m:
                        self.m[id(p)], self.v[id(p)] = torch.zeros_like(p, dtype=torch.float32), torch.zeros_like(p, dtype=torch.float32)
                    m, v = self.m[id(p)], self.v[id(p)]
                    if not (m.is_contiguous() and v.is_contiguous()):
                        m, v = self.m[id(p)], self.v[id(p)] = m.contiguous(), v.contiguous()
                    pd = p.data if p.data.is_contiguous() and p.data_ptr() % 16 == 0 else None       # (else: stepped through a copy)
                    g = p.grad.contiguous().float()
                    work.append(_Work(pd if pd is not None else p.data.contiguous().clone(), g if g.data_ptr() % 16 == 0 else g.clone(), m, v,
                                      copy_back=None if pd is not None else p, group=group_of[id(p)] if grouped else 0))
                continue
            n = plan[1]
            flat = self._flats.get(plan[0])
            if flat is None:
                mf, vf = (torch.zeros((n,), dtype=torch.float32, device=dev) for _ in range(2))
                for p, o in zip(grp, plan[2]):                # carry over moments from per-tensor steps, then keep views
                    for store, fl in ((self.m, mf), (self.v, vf)):
                        view = fl[o:o + p.numel()].view(p.shape)
                        if id(p) in store:
                            view.copy_(store[id(p)])
                        store[id(p)] = view
                flat = self._flats[plan[0]] = (mf, vf)
            pflat = torch.empty(0, dtype=torch.float32, device=dev).set_(grp[0].data.untyped_storage(), 0, (n,))
            gflat = torch.empty(0, dtype=torch.float32, device=dev).set_(grp[0].grad.untyped_storage(), 0, (n,))
            slab = _SLABS.get(plan[0])                        # the trainer's slab these parameters live in: its 16-bit copy is written along
            slab = slab() if slab is not None else None
            if slab is not None and (slab.flat32.data_ptr() != plan[0] or slab.flat16 is None or slab.flat16.numel() != n):
                slab = None
            table, gid = self._segments(grp, plan, group_of) if grouped else (None, 0)
            work.append(_Work(pflat, gflat, flat[0], flat[1], None if slab is None else slab.flat16, slab, table=table, group=gid))
        clip = self.max_grad_norm is not None
        if clip:
            # the norm pass of every work item, partials side by side: it sets the same flag as cir_grads_check, so it replaces that test;
            # cir_adamw_begin_clip then adds ALL partials - one global norm, as clip_grad_norm_ over all parameters
            sizes = [T.grads_sumsq_workspace(w.g.numel()) for w in work]
            if self._partials is None or self._partials.numel() != sum(sizes) or self._partials.device != dev:
                self._partials = torch.empty((sum(sizes),), dtype=torch.float64, device=dev)
            o = 0
            for w, k in zip(work, sizes):
                T.grads_sumsq(w.g, st, self._partials[o:o + k])
                o += k
        elif need:
            for w in work:
                # the trainer's backward tested exactly this buffer and no torch op has written to it since (version counter of the buffer
                # and its views): its flag stands; anything else - accumulated sums, edited gradients, foreign buffers - is tested here
                ck = None if w.slab is None else w.slab.checked
                if ck is not None and ck[0] == w.g.data_ptr() and w.slab.gflat is not None and w.slab.gflat.data_ptr() == ck[0] and w.slab.gflat._version == ck[2]:
                    st[0:1] |= (~ck[1].reshape(1)).to(torch.int32)
                else:
                    T.grads_check(w.g, st)
        if clip:
            T.adamw_begin_clip(st, self.betas, self._partials, self.max_grad_norm)
        else:
            T.adamw_begin(st, self.betas)
        # the applied rate of a group: float32(lr * lr_scale), the product in Python doubles (the entry point takes floats)
        scalars = [(float(np.float32(g["lr"] * g.get("lr_scale", 1.0))), g["weight_decay"], g["eps"]) for g in self.param_groups] if grouped else None
        for w in work:
            if grouped:
                T.adamw_step_groups(w.p, w.g, w.m, w.v, st, scalars, self.betas, table=w.table, group=w.group, clip=clip, p16=w.p16)
            else:
                T.adamw_step_dev(w.p, w.g, w.m, w.v, st, self.lr, self.betas, self.eps, self.wd, p16=w.p16)
            if w.copy_back is not None:                       # (a non-contiguous parameter stepped through a contiguous copy)
                w.copy_back.data.copy_(w.p)
        # the kernels wrote through pointers: move the parameters' version counters, which the packed copies (engines, graphs, K/V banks,
        # slabs) compare - then the slabs whose 16-bit copy was written along record the key as it now is (all of them: a slab marked before
        # a later launch of this step would re-cast at its next step)
        increment_version(ps)
        for w in work:
            if w.slab is not None:
                w.slab.mark_fresh16()                         # (a skipped step leaves both copies as they were: still consistent)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        """torch.optim.AdamW's layout (utils.save_model calls this once per epoch, utils.py:135-150; stage2_train.py:303):
        {"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [group]}, i indexing the requires_grad parameters in constructor
        order.  The moments are the LIVE tensors (on the flat path the views into the slab-sized buffers: torch.save writes each buffer
        once), `step` the one global count of applied steps as torch writes it (0-d fp32, one tensor per entry: torch increments each in
        place).  "cir" carries what torch has no slot for; torch.optim ignores it.  Reads the device (the counts live there)."""
        t = self.t
        state = {i: {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": self.m[id(p)], "exp_avg_sq": self.v[id(p)]}
                 for i, p in enumerate(self.params) if id(p) in self.m}
        groups, o = [], 0
        for g in self.param_groups:                           # torch's layout: global indices in constructor order
            group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
                     "maximize": False, "params": list(range(o, o + len(g["params"])))}
            if "lr_scale" in g:
                group["lr_scale"] = g["lr_scale"]
            groups.append(group)
            o += len(g["params"])
        cir = {"skipped_steps": self.skipped_steps, "format": 1}
        if self.max_grad_norm is not None:
            cir["max_grad_norm"] = self.max_grad_norm
        return {"state": state, "param_groups": groups, "cir": cir}

    def _read_state_dict(self, sd):
        """Validate `sd` against this optimizer without touching it: (groups, {i: (exp_avg, exp_avg_sq)}, applied steps, skipped steps).
        ValueError names the first offender."""
        groups = sd["param_groups"]
        mine = self.param_groups
        if len(groups) != len(mine):
            raise ValueError(f"AdamW.load_state_dict: {len(groups)} parameter groups in the state dict; this optimizer has "
                             + ("exactly one" if len(mine) == 1 else str(len(mine))))
        for k, (group, own) in enumerate(zip(groups, mine)):
            which = "the saved group" if len(mine) == 1 else f"saved group {k}"
            if len(group["params"]) != len(own["params"]):
                raise ValueError(f"AdamW.load_state_dict: {which} has {len(group['params'])} parameters, this optimizer has {len(own['params'])}"
                                 + ("" if len(mine) == 1 else " in that group"))
            for flag in ("amsgrad", "maximize"):
                if group.get(flag, False):
                    raise ValueError(f"AdamW.load_state_dict: {which} has {flag}=True, which cir_adamw_step does not implement")
            if group.get("decoupled_weight_decay", True) is False:
                raise ValueError(f"AdamW.load_state_dict: {which} has decoupled_weight_decay=False (torch.optim.Adam's L2 penalty, not AdamW)")
            if tuple(group["betas"]) != tuple(groups[0]["betas"]):
                raise ValueError(f"AdamW.load_state_dict: saved group {k} has betas {tuple(group['betas'])}, group 0 {tuple(groups[0]['betas'])}; "
                                 "this optimizer shares one pair")
        norm = sd.get("cir", {}).get("max_grad_norm", self.max_grad_norm)
        if norm is not None and not (math.isfinite(norm) and norm > 0):
            raise ValueError(f"AdamW.load_state_dict: max_grad_norm {norm} is not finite and > 0")
        moments, t = {}, None
        for i, entry in sd["state"].items():
            if not isinstance(i, int) or not 0 <= i < len(self.params):
                raise ValueError(f"AdamW.load_state_dict: state entry {i!r} names no parameter (this optimizer has {len(self.params)})")
            for key in ("exp_avg", "exp_avg_sq"):
                if tuple(entry[key].shape) != tuple(self.params[i].shape):
                    raise ValueError(f"AdamW.load_state_dict: {key} of parameter {i} has shape {tuple(entry[key].shape)}, "
                                     f"the parameter {tuple(self.params[i].shape)}")
            step = float(entry["step"])                       # a tensor on any device, an int or a float
            if step != int(step) or step < 0:
                raise ValueError(f"AdamW.load_state_dict: step of parameter {i} is {step}")
            if t is not None and int(step) != t:
                raise ValueError(f"AdamW.load_state_dict: parameter {i} is at step {int(step)}, the parameters before it at step {t}; "
                                 "this optimizer keeps one count for all of them")
            t = int(step)
            moments[i] = (entry["exp_avg"], entry["exp_avg_sq"])
        return groups, moments, t or 0, int(sd.get("cir", {}).get("skipped_steps", 0))

    @torch.no_grad()
    def load_state_dict(self, sd: dict):
        """Continue from `state_dict()`'s output or from a torch.optim.AdamW state dict (the same groups, no amsgrad / maximize).  Everything is
        checked before anything changes (ValueError).  The moments are COPIED, as contiguous fp32 on their parameter's device: into the
        views of the flat buffers where those exist, otherwise into per-tensor moments that the first flat step carries into its buffers
        (step() above, one group per slab).  The hyperparameters come from the saved group, as in torch.  The applied / skipped counts go
        into the device state; cir_adamw_begin recomputes both bias corrections from the count at every step, so nothing else is carried.
        A parameter without an entry keeps no moments.  Call it with the parameters on the device they train on."""
        groups, moments, t, skipped = self._read_state_dict(sd)
        flat_storages = {f.untyped_storage().data_ptr() for pair in self._flats.values() for f in pair}
        for i, p in enumerate(self.params):
            for store, k in ((self.m, 0), (self.v, 1)):
                cur = store.get(id(p))
                if i in moments:
                    if cur is None:
                        cur = store[id(p)] = torch.empty(p.shape, dtype=torch.float32, device=p.device)
                    cur.copy_(moments[i][k])
                elif cur is not None:
                    if cur.untyped_storage().data_ptr() in flat_storages:     # (a slice of a flat buffer cannot leave it: zero = no history)
                        cur.zero_()
                    else:
                        del store[id(p)]
        for g, group in zip(self.param_groups, groups):
            g["lr"], g["betas"], g["eps"], g["weight_decay"] = group["lr"], tuple(group["betas"]), group["eps"], group["weight_decay"]
            if "lr_scale" in group:
                g["lr_scale"] = group["lr_scale"]
            else:
                g.pop("lr_scale", None)
        g = self.param_groups[0]
        self.betas, self.eps, self.wd = g["betas"], g["eps"], g["weight_decay"]          # (what the one-group step() reads)
        self.max_grad_norm = sd.get("cir", {}).get("max_grad_norm", self.max_grad_norm)
        if self._state is None:
            dev = self.params[0].device if self.params else torch.device("cpu")
            self._state = torch.zeros((8,), dtype=torch.int32, device=dev)
        self._state[0:3] = torch.tensor([0, t, skipped], dtype=torch.int32)
