"""tests/optim_group_cases.py on the CPU: a correct fp32 stand-in passes every scenario, each wrong form fails on a named one, the rule
agrees with torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with groups; and the host logic of train_optim.AdamW with several parameter
groups: constructor forms and refusals, state dicts exchanged with torch in both directions, refusals that change nothing, the four
schedules on both optimizers, train.param_groups on the tiny stage-II and stage-I models.  Nothing here launches a kernel."""
import copy
import math

import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import config, synthetic, train
from candidate_reranking_cir_amd.train import AdamW
from tests import optim_cases as O
from tests import optim_group_cases as G


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("name", sorted(G.SCENARIOS))
def test_correct_standin_passes(name):
    scn = G.SCENARIOS[name]
    fails = G.check(scn, *G.standin(scn))
    assert not fails, fails[:5]


# the scenario on which each wrong form must fail
NAMED = {"coef_no_eps": "tiny_norm", "coef_no_clamp": "clip_inactive", "norm_per_item": "clip_active", "clip_update": "clip_active",
         "boundary_early": "clip_active", "boundary_late": "clip_active", "lr_scale_ignored": "no_clip", "wd_of_previous": "no_clip",
         "norm_fp32": "huge"}


def test_every_wrong_form_is_named():
    assert set(NAMED) == set(G.WRONG)


@pytest.mark.parametrize("wrong", G.WRONG)
def test_wrong_form_fails(wrong):
    scn = G.SCENARIOS[NAMED[wrong]]
    assert G.check(scn, *G.standin(scn, wrong)), (wrong, scn)


def test_scenarios_cover_what_they_claim():
    for scn in G.SCENARIOS.values():
        norm, coef, _ = G.reference(scn)                              # (asserts the range rule on the clipped gradient)
        assert np.isfinite(norm) and norm > 0
    assert G.reference(G.SCENARIOS["clip_inactive"])[1] == np.float32(1.0)
    assert 0.99 < G.reference(G.SCENARIOS["clip_at"])[1] <= 1.0           # (1e-6 may vanish beside the norm in fp32)
    assert 0.4 < G.reference(G.SCENARIOS["clip_active"])[1] <= 0.5
    c = G.reference(G.SCENARIOS["tiny_norm"])[1]
    n = G.reference(G.SCENARIOS["tiny_norm"])[0]
    assert c < 1.0 and float(n) < 1e-5 and abs(c - 1e-6 / float(n)) > 0.05 * c       # the + 1e-6 changes the coefficient by more than 5 %
    huge = G.SCENARIOS["huge"].inputs()
    with np.errstate(over="ignore"):
        assert np.isinf(np.square(huge[0]["g"].numpy()).sum(dtype=np.float32)) and np.isfinite(G.reference(G.SCENARIOS["huge"])[0])
    ends = G.seg_ends(G.SEG_LENGTHS)
    assert sorted(G.SEG_LENGTHS) == [8, 16, 2040, 2048, 2056]
    assert any(e < 2048 for e in ends) and 2048 in ends and any(e > 2048 and e % 2048 for e in ends)
    ends_b = G.seg_ends(G.SEG_LENGTHS_B)
    assert any(0 < (e // 4) % 512 < 256 for e in ends[:-1]) and all(256 < (e // 4) % 512 < 511 for e in ends_b[:-1])    # both float4 of a thread
    assert len(G.SCENARIOS["eight_groups"].groups) == 8
    assert G.ulps32(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1 and G.ulps32(np.float32(-0.0), np.float32(0.0)) == 0


def test_rule_agrees_with_torch_clip_and_grouped_adamw():
    """clip_grad_norm_ + torch.optim.AdamW with the same groups (fp32-rounded scalars; torch knows no lr_scale: its lr is the applied rate).
    torch takes the norm in fp32 - per tensor, then the norm of the K norms - and forms the coefficient as reciprocal times max_norm, so its
    clipped gradient is not ours bit for bit.  A priori: each per-tensor sum of N_k squares is within N_k u relative, the root halves that and
    adds u, the K squares and their sum add (K + 1) u halved, the last root u, the coefficient's sum, reciprocal and product 3 u, the product
    with g one more: torch's g_c is within (max N_k / 2 + K / 2 + 8) u of g * coef, ours within 3 u.  Then the STEP is compared exactly as
    the kernels' is: from torch's own clipped gradient, within optim_cases' bound, per element with its group's scalars."""
    scn = G.SCENARIOS["clip_active"]
    norm, coef, _ = G.reference(scn)
    sc = G.applied(scn.groups)
    for item in scn.inputs():
        # one tensor per segment, so that every parameter lies in one group
        bounds = list(zip([0] + item["ends"][:-1], item["ends"]))
        ps = [torch.nn.Parameter(item["p"][a:b].clone()) for a, b in bounds]
        for p, (a, b) in zip(ps, bounds):
            p.grad = item["g"][a:b].clone()
        tgroups = [dict(params=[p for p, k in zip(ps, item["ids"]) if k == gid], lr=lr, weight_decay=wd, eps=eps) for gid, (lr, wd, eps) in enumerate(sc)]
        opt = torch.optim.AdamW([g for g in tgroups if g["params"]], betas=(G.B1, G.B2))
        for p, (a, b) in zip(ps, bounds):
            st = opt.state[p]
            st["step"] = torch.tensor(float(scn.t - 1))
            st["exp_avg"], st["exp_avg_sq"] = item["m"][a:b].clone(), item["v"][a:b].clone()
        max_norm = float(G.norm32([item["g"].numpy()])) * 0.5           # (this item alone is torch's whole step)
        own_coef = G.coef32(G.norm32([item["g"].numpy()]), max_norm)
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        k_tensors, n_max = len(ps), max(p.numel() for p in ps)
        assert abs(float(total) - float(G.norm32([item["g"].numpy()]))) <= (n_max / 2 + k_tensors / 2 + 3) * O.U * float(total)
        gc = torch.cat([p.grad for p in ps])
        assert bool(((gc.double() - item["g"].double() * float(own_coef)).abs() <= (n_max / 2 + k_tensors / 2 + 8) * O.U * gc.double().abs()).all())
        opt.step()
        ref, bnd = G.group_step_terms(item["p"], gc, item["m"], item["v"], item["egroups"], sc, scn.t, None)
        out = dict(p=torch.cat([p.detach() for p in ps]), m=torch.cat([opt.state[p]["exp_avg"] for p in ps]),
                   v=torch.cat([opt.state[p]["exp_avg_sq"] for p in ps]))
        fails = G.check_step("torch", out, ref, bnd)
        assert not fails, fails[:5]


# ------------------------------------------------------------------------------------------------ train_optim.AdamW on the host
SHAPES = [(3, 4), (5,), (2, 3, 2), (), (7,), (4, 2)]
KW = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]


def _groups(ps):
    return [{"params": ps[0:2]}, {"params": ps[2:3], "weight_decay": 0.0, "eps": 1e-6}, {"params": ps[3:], "lr": 5e-4, "lr_scale": 0.1}]


def _twin(ps):
    return [torch.nn.Parameter(p.detach().clone()) for p in ps]


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b and type(a) is type(b)


def test_constructor_forms():
    ps = _params()
    one = AdamW(ps, **KW)
    assert len(one.param_groups) == 1 and one.param_groups[0]["params"] is one.params and not one._grouped() and one.max_grad_norm is None
    assert set(one.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}
    opt = AdamW(_groups(ps), max_grad_norm=1.0, **KW)
    g = opt.param_groups
    assert [len(x["params"]) for x in g] == [2, 1, 3] and [id(p) for p in opt.params] == [id(p) for p in ps] and opt._grouped()
    assert (g[0]["lr"], g[0]["weight_decay"], g[0]["eps"]) == (1e-3, 0.05, 1e-7) and "lr_scale" not in g[0]
    assert (g[1]["lr"], g[1]["weight_decay"], g[1]["eps"]) == (1e-3, 0.0, 1e-6)
    assert (g[2]["lr"], g[2]["weight_decay"], g[2]["lr_scale"]) == (5e-4, 0.05, 0.1)
    assert opt.lr == 1e-3
    opt.lr = 2e-3
    assert g[0]["lr"] == 2e-3 and g[2]["lr"] == 5e-4                                           # opt.lr means group 0
    assert opt.grad_norm == 0.0 and opt.clip_coef == 1.0 and opt.t == 0                       # before the first step
    # a single tensor as a group's "params", a frozen parameter left out, one group with an lr_scale takes the segmented path
    ps[1].requires_grad_(False)
    lone = AdamW([{"params": ps[0]}, {"params": ps[1:3]}], **KW)
    assert [len(x["params"]) for x in lone.param_groups] == [1, 1]
    assert AdamW([{"params": ps[:1], "lr_scale": 0.5}], **KW)._grouped() and AdamW(ps[:1], max_grad_norm=2.0)._grouped()
    # the caller's dicts are not written to
    mine = _groups(_params())
    keys = [set(x) for x in mine]
    AdamW(mine, **KW)
    assert [set(x) for x in mine] == keys


def test_constructor_refusals():
    ps = _params()
    with pytest.raises(ValueError, match="more than one parameter group"):
        AdamW([{"params": ps[:2]}, {"params": ps[1:]}], **KW)
    with pytest.raises(ValueError, match="at most 8"):
        AdamW([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(9)], **KW)
    with pytest.raises(ValueError, match="empty parameter list"):
        AdamW([], **KW)
    with pytest.raises(ValueError, match="betas"):
        AdamW([{"params": ps[:2]}, {"params": ps[2:], "betas": (0.9, 0.999)}], **KW)
    AdamW([{"params": ps[:2]}, {"params": ps[2:], "betas": (0.9, 0.98)}], **KW)                # the shared pair, restated: fine
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm"):
            AdamW(ps, max_grad_norm=bad, **KW)
    assert len(AdamW([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(8)], **KW).param_groups) == 8


def _torch_stepped(ps, steps=2):
    gs = _groups(ps)
    for g in gs:                                                                               # torch knows no lr_scale but carries the key
        g.setdefault("lr_scale", 1.0)
    ref = torch.optim.AdamW(gs, **KW)
    for k in range(steps):
        gen = torch.Generator().manual_seed(100 + k)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    return ref


def test_three_group_state_dict_from_torch_and_back():
    ps = _params()
    ref = _torch_stepped(ps)
    ref.param_groups[1]["lr"] = 7e-4
    sd = ref.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2], [3, 4, 5]]
    opt = AdamW(_groups(_twin(ps)), lr=1.0, betas=(0.9, 0.98), eps=1.0, weight_decay=0.3, max_grad_norm=2.5)
    assert opt.state_dict()["state"] == {}
    opt.load_state_dict(sd)
    out = opt.state_dict()
    assert [g["params"] for g in out["param_groups"]] == [[0, 1], [2], [3, 4, 5]]
    for g, rg in zip(out["param_groups"], sd["param_groups"]):
        for key in ("lr", "eps", "weight_decay", "lr_scale"):
            assert g[key] == rg[key], key
        assert tuple(g["betas"]) == tuple(rg["betas"]) and g["amsgrad"] is False and g["maximize"] is False
    assert out["param_groups"][1]["lr"] == 7e-4 and out["param_groups"][2]["lr_scale"] == 0.1
    for i in range(len(SHAPES)):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(out["state"][i][key], sd["state"][i][key])
        assert float(out["state"][i]["step"]) == 2.0
    assert opt.t == 2 and out["cir"] == {"skipped_steps": 0, "format": 1, "max_grad_norm": 2.5}
    # ... and torch continues from ours: a step of both torch optimizers from the two state dicts gives the same parameters
    qs = _twin(ps)
    cont = torch.optim.AdamW(_groups(qs), **KW)
    cont.load_state_dict(out)
    assert cont.param_groups[2]["lr_scale"] == 0.1 and cont.param_groups[1]["lr"] == 7e-4
    gen = torch.Generator().manual_seed(5)
    for p, q in zip(ps, qs):
        p.grad = torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    ref.step(); cont.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, qs))
    # a round trip through our own optimizer keeps everything, max_grad_norm included
    again = AdamW(_groups(_twin(ps)), **KW)
    again.load_state_dict(copy.deepcopy(out))
    assert _same(again.state_dict(), out) and again.max_grad_norm == 2.5
    # without lr_scale in the saved group the key leaves the group, as torch replaces its groups by the saved ones
    del out["param_groups"][2]["lr_scale"]
    again.load_state_dict(out)
    assert "lr_scale" not in again.param_groups[2]


def test_one_group_without_clipping_is_todays_state_dict():
    ps = _params()
    opt = AdamW(ps, **KW)
    sd = opt.state_dict()
    assert sd["cir"] == {"skipped_steps": 0, "format": 1} and len(sd["param_groups"]) == 1
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "params"]


def _bad_cases():
    def group_count(sd):
        sd["param_groups"].pop()

    def one_group(sd):
        del sd["param_groups"][1:]

    def param_count(sd):
        sd["param_groups"][2]["params"].pop()
        sd["param_groups"][1]["params"].append(5)

    def betas_differ(sd):
        sd["param_groups"][1]["betas"] = (0.5, 0.5)

    def amsgrad(sd):
        sd["param_groups"][2]["amsgrad"] = True

    def bad_norm(sd):
        sd["cir"] = {"max_grad_norm": -1.0}

    def moment_shape(sd):
        sd["state"][4]["exp_avg"] = torch.zeros(3)
    return [(group_count, "2 parameter groups in the state dict; this optimizer has 3"), (one_group, "1 parameter groups"),
            (param_count, "saved group 1 has 2 parameters, this optimizer has 1"), (betas_differ, "saved group 1 has betas"), (amsgrad, "amsgrad"),
            (bad_norm, "max_grad_norm"), (moment_shape, "exp_avg of parameter 4")]


@pytest.mark.parametrize("spoil,message", _bad_cases(), ids=[f.__name__ for f, _ in _bad_cases()])
def test_refusals_change_nothing(spoil, message):
    ps = _params()
    opt = AdamW(_groups(_twin(ps)), max_grad_norm=3.0, **KW)
    opt.load_state_dict(_torch_stepped(ps, 2).state_dict())
    sd = copy.deepcopy(_torch_stepped(_params(1), 3).state_dict())        # a state dict that WOULD change every moment, the count and lr
    for g in sd["param_groups"]:
        g["lr"] = 9e-9
    spoil(sd)
    before = copy.deepcopy(opt.state_dict())
    with pytest.raises(ValueError, match=message):
        opt.load_state_dict(sd)
    assert _same(opt.state_dict(), before) and opt.t == 2 and opt.max_grad_norm == 3.0


def test_a_three_group_state_dict_is_refused_by_a_one_group_optimizer():
    ps = _params()
    sd = _torch_stepped(ps).state_dict()
    with pytest.raises(ValueError, match="3 parameter groups in the state dict; this optimizer has exactly one"):
        AdamW(_twin(ps), **KW).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ the schedules
def _both():
    ps, qs = _params(), _params()
    return AdamW(_groups(ps), **KW), torch.optim.AdamW(_groups(qs), **KW)


def test_schedules_on_both_optimizers():
    for opt in _both():
        init_lr, min_lr = 2e-5, 1e-6
        for epoch in range(4):
            lr = train.cosine_lr_schedule(opt, epoch, 4, init_lr, min_lr)
            assert lr == (init_lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * epoch / 4)) + min_lr
            assert all(g["lr"] == lr for g in opt.param_groups)
        for step in (0, 10, 3000, 5000):
            lr = train.warmup_lr_schedule(opt, step, 3000, 1e-6, 2e-5)
            assert lr == min(2e-5, 1e-6 + (2e-5 - 1e-6) * step / 3000) and all(g["lr"] == lr for g in opt.param_groups)
        assert train.warmup_lr_schedule(opt, 5000, 3000, 1e-6, 2e-5) == 2e-5
        for epoch in (0, 1, 7, 200):
            lr = train.step_lr_schedule(opt, epoch, 2e-5, 1e-6, 0.9)
            assert lr == max(1e-6, 2e-5 * (0.9 ** epoch)) and all(g["lr"] == lr for g in opt.param_groups)
        assert train.step_lr_schedule(opt, 200, 2e-5, 1e-6, 0.9) == 1e-6
        for k, g in enumerate(opt.param_groups):
            g["lr"] = 1e-3 * (k + 1)
        assert train.exp_lr_schedule(opt, 3, 0.5) is None                                      # every group's OWN lr times gamma
        assert [g["lr"] for g in opt.param_groups] == [1e-3 * (k + 1) * 0.5 for k in range(3)]
        assert opt.param_groups[2]["lr_scale"] == 0.1 and "lr_scale" not in opt.param_groups[0]     # the ratio between groups survives


def test_applied_rate_is_float32_of_lr_times_lr_scale():
    opt, _ = _both()
    train.cosine_lr_schedule(opt, 1, 4, 2e-5, 1e-6)
    lr = opt.param_groups[2]["lr"]
    assert G.applied(opt.param_groups)[2][0] == float(np.float32(lr * 0.1))                   # the product in doubles, ONE rounding
    assert G.applied(opt.param_groups)[0][0] == float(np.float32(lr))


# ------------------------------------------------------------------------------------------------ train.param_groups
def _tiny_models():
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    g = config.BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256, encoder_width=128)
    v = config.VitGeometry(image_size=64, width=128, depth=2, num_heads=2)
    return (BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()),
            BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()))


@pytest.mark.parametrize("which", [0, 1], ids=["stage2", "stage1"])
def test_param_groups_partition(which):
    model = _tiny_models()[which]
    frozen = next(p for n, p in model.named_parameters() if n.endswith("mlp.fc1.weight"))
    frozen.requires_grad_(False)
    named = {id(p): n for n, p in model.named_parameters()}
    plain = train.param_groups(model, 0.05)
    assert [g["weight_decay"] for g in plain] in ([0.0, 0.05], [0.05, 0.0]) and all("lr_scale" not in g for g in plain)
    groups = train.param_groups(model, 0.05, {"visual_encoder.": 0.1})
    assert len(groups) == 4
    got = [id(p) for g in groups for p in g["params"]]
    want = [id(p) for p in model.parameters() if p.requires_grad]
    assert len(got) == len(set(got)) and sorted(got) == sorted(want) and id(frozen) not in got
    for g in groups:
        names = [named[id(p)] for p in g["params"]]
        vis = [n.startswith("visual_encoder.") for n in names]
        assert all(vis) or not any(vis)
        assert (g.get("lr_scale") == 0.1) == all(vis) and ("lr_scale" in g) == all(vis)
        for n, p in zip(names, g["params"]):
            nodecay = p.ndim <= 1 or n in ("visual_encoder.pos_embed", "visual_encoder.cls_token")
            assert g["weight_decay"] == (0.0 if nodecay else 0.05), n
    flat = [n for g in groups for n in (named[id(p)] for p in g["params"])]
    assert "visual_encoder.pos_embed" in flat and "visual_encoder.cls_token" in flat
    # deterministic in order, accepted by both optimizers (torch first writes its defaults into the dicts it is given: fresh ones each)
    again = train.param_groups(model, 0.05, {"visual_encoder.": 0.1})
    assert [[id(p) for p in g["params"]] for g in again] == [[id(p) for p in g["params"]] for g in groups]
    for g in groups:                                                  # within a group: named_parameters() order
        order = [list(named).index(id(p)) for p in g["params"]]
        assert order == sorted(order)
    ours = AdamW(groups, lr=2e-5, max_grad_norm=1.0)
    theirs = torch.optim.AdamW(again, lr=2e-5)
    assert [len(g["params"]) for g in ours.param_groups] == [len(g["params"]) for g in theirs.param_groups]
    assert [g.get("lr_scale") for g in theirs.param_groups] == [g.get("lr_scale") for g in ours.param_groups]
