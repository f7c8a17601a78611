"""Resuming a training run from a checkpoint on a real MI355X: `model.state_dict()`, `train.AdamW.state_dict()` and
`train.training_state(model)` written with torch.save, read back with torch.load(weights_only=True) into a NEW model and a NEW optimizer,
continue the run bit for bit under the deterministic mode - for the stage-II fusion pass (dropout sites numbered by the trainer's counters),
the stage-I pass (one draw from torch's generator per forward) and ViT fine-tuning (two parameter slabs, DropPath numbered by the ViT
trainer's counters); the applied / skipped step counts survive; torch.optim.AdamW's state continues on the hand-written step and back.

Shapes: tests/test_train_deterministic_gpu.py's - thirteen captions (L = 15), 17 image tokens, dropout 0.1 / 0.1: a ragged third workgroup in
every row kernel and a tail in every weight gradient.  Between the save and the load every resumed run re-seeds torch's generator with
another value, as a new process would find it."""
import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests.test_train_gpu import BF, HF, build, freeze_vit

pytestmark = pytest.mark.gpu
B = 13
CAPS = [synthetic.caption_text(300 + i, 9 + i % 5) for i in range(B)]
KW = dict(lr=2e-5, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture
def mode():
    from candidate_reranking_cir_amd import train
    assert train.deterministic() is False
    yield train.set_deterministic
    train.set_deterministic(False)


def _optimizer(model):
    from candidate_reranking_cir_amd.train import AdamW
    return AdamW([p for p in model.parameters() if p.requires_grad], model=model, **KW)


def _result(model, opt):
    """({name: parameter}, {name: first moment}, {name: second moment}) of every parameter the optimizer holds moments for."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert any(id(p) in opt.m for _, p in named)
    return ({n: p.detach().clone() for n, p in named}, {n: opt.m[id(p)].clone() for n, p in named if id(p) in opt.m},
            {n: opt.v[id(p)].clone() for n, p in named if id(p) in opt.v})


def _differences(a, b):
    out = []
    for what, x, y in zip(("parameter", "first moment", "second moment"), a, b):
        assert x.keys() == y.keys() and len(x) > 50
        out += [(what, n) for n in x if not torch.equal(x[n], y[n])]
    return out


def _save(path, model, opt):
    from candidate_reranking_cir_amd import train
    torch.save({"model": model.state_dict(), "optimizer_state_dict": opt.state_dict(), "training_state": train.training_state(model)}, str(path))


def _resume(path, model, with_training_state=True):
    """A new optimizer for the new `model`, both continued from the file: model, optimizer, training state - in that order."""
    from candidate_reranking_cir_amd import train
    torch.manual_seed(987654321)                                     # (a new process starts from some other generator state)
    ck = torch.load(str(path), weights_only=True)
    model.load_state_dict(ck["model"], strict=True)
    opt = _optimizer(model)
    opt.load_state_dict(ck["optimizer_state_dict"])
    if with_training_state:
        train.load_training_state(model, ck["training_state"])
    return opt


def _run_resumed(new_model, steps, first, total, path, control=False):
    """Run A: `total` steps.  Run B: `first` steps, save, new model + optimizer from the file, the rest.  Returns [A, B(, B resumed without the
    training state)] as `_result` triples."""
    torch.manual_seed(77)
    ma = new_model()
    oa = _optimizer(ma)
    steps(ma, oa, total)
    assert oa.t == total and oa.skipped_steps == 0
    a = _result(ma, oa)
    torch.manual_seed(77)
    mb = new_model()
    ob = _optimizer(mb)
    steps(mb, ob, first)
    _save(path, mb, ob)
    del mb, ob
    out = [a]
    for with_state in ((True, False) if control else (True,)):
        mb = new_model()
        ob = _resume(path, mb, with_state)
        assert ob.t == first
        steps(mb, ob, total - first)
        assert ob.t == total and ob.skipped_steps == 0
        out.append(_result(mb, ob))
    return out


def _geometry():
    _, g, v, _, _ = H.tiny_setup()
    assert (g.hidden_dropout_prob, g.attention_probs_dropout_prob) == (0.1, 0.1)
    return g, v


def _stage2_model(dtype, frozen=True):
    zf, g, v, _, _ = H.tiny_setup()
    m2, _ = build(g, v, int(zf["seed"]), str(zf["profile"]), dtype)
    if frozen:
        freeze_vit(m2)
    return m2.train()


def _stage2_inputs(g, seed=9):
    l = H.tokenize(CAPS)[0].shape[1]
    assert l == 15
    rng = torch.Generator().manual_seed(seed)
    return torch.randn((B, l, g.hidden_size), generator=rng).cuda(), torch.randn((B, 17, g.encoder_width), generator=rng).cuda()


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_g1_stage2_run_resumes_bit_for_bit(cuda, mode, dtype, tmp_path):
    mode(True)
    g, _ = _geometry()
    z_t, feats = _stage2_inputs(g)

    def steps(m2, opt, k):
        for _ in range(k):
            opt.zero_grad()
            F.cross_entropy(m2.img_txt_fusion(z_t, feats, CAPS), torch.arange(B, device=cuda)).backward()
            opt.step()
    a, b, c = _run_resumed(lambda: _stage2_model(dtype), steps, 2, 4, tmp_path / "ck.pt", control=True)
    assert not _differences(a, b), _differences(a, b)[:5]
    assert any(bool(t.any()) for t in a[1].values())
    # control: without the training state the dropout masks of steps 0, 1 are replayed - the test sees the counters
    assert any(what == "parameter" for what, _ in _differences(a, c))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_g2_stage1_run_resumes_bit_for_bit(cuda, mode, dtype, tmp_path):
    """MedTrainer draws one base seed per forward from torch's global generator: this is the case that rests on its saved state."""
    from tests.test_train_stage1_gpu import TINY, TINY_VIT, build as build1
    mode(True)
    g, v = H.geometry(dict(TINY, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), TINY_VIT)
    gen = torch.Generator().manual_seed(33)
    ref = torch.randn((B, 17, g.encoder_width), generator=gen).cuda()
    tgt = F.normalize(torch.randn((B + 2, 256), generator=gen), dim=-1).cuda()
    seeds = []

    def steps(m1, opt, k):
        for _ in range(k):
            opt.zero_grad()
            F.cross_entropy(m1.img_txt_fusion(ref, tgt, CAPS), torch.arange(B, device=cuda)).backward()
            seeds.append(m1._trainer.last_seed)
            opt.step()
    a, b, c = _run_resumed(lambda: build1(g, v, 7, "test", dtype)[0].train(), steps, 2, 4, tmp_path / "ck.pt", control=True)
    assert seeds[0:4] == seeds[4:8] and len(set(seeds[0:4])) == 4 and seeds[8:10] != seeds[2:4]        # A; B; the control's draws differ
    assert not _differences(a, b), _differences(a, b)[:5]
    assert "temp" in a[1] and any(what == "parameter" for what, _ in _differences(a, c))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_g3_vit_fine_tuning_run_resumes_bit_for_bit(cuda, mode, dtype, tmp_path):
    """--blip-img-tune: two slabs (two-branch encoder, ViT), two counted trainers; the loaded per-tensor moments are carried into BOTH
    flat moment buffers at the first flat step."""
    mode(True)
    g, v = _geometry()
    z_t, _ = _stage2_inputs(g, seed=4)
    images = synthetic.scene_images(range(40, 40 + B), v.image_size).cuda()
    opts = []

    def steps(m2, opt, k):
        for _ in range(k):
            opt.zero_grad()
            feats = m2.img_embed(images)
            assert feats.requires_grad
            F.cross_entropy(m2.img_txt_fusion(z_t, feats.float(), CAPS, train=True), torch.arange(B, device=cuda)).backward()
            opt.step()
        opts.append(opt)
    a, b = _run_resumed(lambda: _stage2_model(dtype, frozen=False), steps, 2, 3, tmp_path / "ck.pt")
    assert all(len(o._flats) == 2 for o in opts)
    assert not _differences(a, b), _differences(a, b)[:5]
    assert sum(n.startswith("visual_encoder.") for n in a[1]) == 6 + 12 * v.depth
    assert (opts[-1].model._trainer.step_no, opts[-1].model._vit_trainer.step_no) == (3, 3)


def test_g4_skipped_step_counts_survive(cuda, mode, tmp_path):
    mode(True)
    g, _ = _geometry()
    z_t, feats = _stage2_inputs(g)

    def step(m2, opt, spoil=False):
        opt.zero_grad()
        F.cross_entropy(m2.img_txt_fusion(z_t, feats, CAPS), torch.arange(B, device=cuda)).backward()
        if spoil:
            dict(m2.named_parameters())["cls_head.0.weight"].grad.view(-1)[3] = float("inf")
        opt.step()
    torch.manual_seed(78)
    m2 = _stage2_model(HF)
    opt = _optimizer(m2)
    step(m2, opt)
    after_one = _result(m2, opt)
    step(m2, opt, spoil=True)
    assert opt.t == 1 and opt.skipped_steps == 1
    assert not _differences(after_one, _result(m2, opt))             # the skipped step applied nothing
    _save(tmp_path / "ck.pt", m2, opt)
    sd = opt.state_dict()
    assert sd["cir"] == {"skipped_steps": 1, "format": 1} and all(float(e["step"]) == 1.0 for e in sd["state"].values())
    m3 = _stage2_model(HF)
    opt3 = _resume(tmp_path / "ck.pt", m3)
    assert opt3.t == 1 and opt3.skipped_steps == 1
    step(m2, opt)                                                    # the uninterrupted twin's next step
    step(m3, opt3)
    assert (opt.t, opt.skipped_steps) == (2, 1) == (opt3.t, opt3.skipped_steps)
    assert not _differences(_result(m2, opt), _result(m3, opt3))
    assert _differences(after_one, _result(m3, opt3))


def test_g5_interchange_with_torch_adamw(cuda):
    """tests/test_train_gpu.py::test_flat_adamw_matches_torch_adamw's setting and bound (2e-6 after three steps of the two implementations
    on the same gradients), with the state handed over after the second step: torch -> train.AdamW on the flat and on the per-tensor path,
    then train.AdamW -> torch."""
    from candidate_reranking_cir_amd.train import AdamW
    zf, g, v, _, _ = H.tiny_setup()
    m = build(g, v, int(zf["seed"]), str(zf["profile"]), BF)[0]
    freeze_vit(m)
    m.train()
    caps = [synthetic.caption_text(90 + i, n) for i, n in enumerate((4, 8, 6))]
    rng = torch.Generator().manual_seed(3)
    l = H.tokenize(caps)[0].shape[1]
    z_t = torch.randn((3, l, g.hidden_size), generator=rng).cuda()
    feats = torch.randn((3, 17, g.encoder_width), generator=rng).cuda()
    F.cross_entropy(m.img_txt_fusion(z_t, feats, caps), torch.arange(3, device=cuda)).backward()
    ps = [p for p in m.parameters() if p.grad is not None]
    assert len(ps) > 300
    kw = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    start = [p.detach().clone() for p in ps]

    def twins(values):
        qs = [x.detach().clone().requires_grad_(True) for x in values]
        for q, p in zip(qs, ps):
            q.grad = p.grad.clone()
        return qs

    def worst(xs, ys):
        return max((x.data - y.data).abs().max().item() for x, y in zip(xs, ys))
    # torch -> ours
    rs = twins(start)
    ref = torch.optim.AdamW(rs, **kw)
    ref.step(); ref.step()
    qs = twins(rs)
    for p, r in zip(ps, rs):
        p.data.copy_(r.data)                                         # (in place: the parameters stay slices of the trainer's slab)
    ours_flat, ours_each = AdamW(ps, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0), AdamW(qs, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0)
    ours_flat.load_state_dict(ref.state_dict())
    ours_each.load_state_dict(ref.state_dict())
    assert not ours_flat._flats and ours_flat.t == 2 == ours_each.t
    ours_flat.step(); ours_each.step(); ref.step()
    assert len(ours_flat._flats) == 1 and not ours_each._flats and ours_flat.t == 3 == ours_each.t
    moved = worst(ps, start)
    e_flat, e_each = worst(ps, rs), worst(qs, rs)
    print(f"\n[torch -> train.AdamW after 2 steps, third step] largest update {moved:.3e}; flat path max diff {e_flat:.3e}, per-tensor path {e_each:.3e}")
    assert moved > 2e-3 and e_flat < 2e-6 and e_each < 2e-6
    # a load into an optimizer whose flat buffers exist copies into their views
    (mf, vf), = ours_flat._flats.values()
    ours_flat.load_state_dict(ref.state_dict())
    sd = ref.state_dict()["state"]
    for i, p in enumerate(ps):
        assert ours_flat.m[id(p)].untyped_storage().data_ptr() == mf.untyped_storage().data_ptr()
        assert ours_flat.v[id(p)].untyped_storage().data_ptr() == vf.untyped_storage().data_ptr()
        assert torch.equal(ours_flat.m[id(p)], sd[i]["exp_avg"]) and torch.equal(ours_flat.v[id(p)], sd[i]["exp_avg_sq"])
    # ours -> torch
    for p, s in zip(ps, start):
        p.data.copy_(s)
    qs = twins(start)
    for name, mine, opt in (("flat", ps, AdamW(ps, **kw)), ("per-tensor", qs, AdamW(qs, **kw))):
        opt.step(); opt.step()
        sd = opt.state_dict()
        copied = {"state": {i: {k: t.clone() for k, t in e.items()} for i, e in sd["state"].items()}, "param_groups": sd["param_groups"], "cir": sd["cir"]}
        ts = twins(mine)
        theirs = torch.optim.AdamW(ts, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0)
        theirs.load_state_dict(copied)
        opt.step(); theirs.step()
        e = worst(mine, ts)
        print(f"[train.AdamW ({name}) -> torch after 2 steps, third step] max diff {e:.3e}")
        assert opt.t == 3 and bool((len(opt._flats) == 1) == (name == "flat")) and e < 2e-6
        assert all(float(s["step"]) == 3.0 for s in theirs.state_dict()["state"].values())
