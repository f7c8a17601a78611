"""explain.cross_attention_maps / gradcam and the rectangular NlvrTrainer on a real MI355X, at the tiny geometry of helpers.tiny_setup()
(128 wide, 2 heads, 8 layers: both merge variants; 17 image tokens), ragged captions, B = 2 queries x Bt = 3 candidates.

The oracle is torch autograd through oracle.cir_oracle.nlvr_forward + cls_head composed here for a rectangular batch, with a `drop=`
recorder that returns its input unchanged and keeps the "cross_attn" probabilities with retain_grad(), and `relu_mask` from the trainer's
head_mask() (the piece of cls_head's ReLU the forward under test took).  The maps are compared per (layer, branch) in relative L2 under
GRAD_REL of tests/test_train_gpu.py - the project's worst-tensor cap for gradients of this same pass at this geometry; `grads` is made from
the very dO whose products those gradients are.  That is a PLUMBING check (a wrong pair, branch, layer or scale gives an error near 1); the
sharp arithmetic check is the op-level table (tests/test_attn_maps_gpu.py).  `pytest -s` prints the measured values (LABNOTES section 34)."""
import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests.test_train_gpu import BF, GRAD_REL, HF, build, freeze_vit

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LAYERS = (0, 7)
B_N, BT_N = 2, 3


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _inputs(g, b=B_N, bt=BT_N, seed=11, lens=(4, 7, 5)):
    caps = [synthetic.caption_text(70 + i, n) for i, n in enumerate(lens[:b])]
    ids, mask = H.tokenize(caps)
    ids = ids.clone()
    ids[:, 0] = synthetic.HashTokenizer().enc_token_id
    gen = torch.Generator().manual_seed(seed)
    z_t = torch.randn((b, ids.shape[1], g.hidden_size), generator=gen)
    feats = torch.randn((bt, 17, g.encoder_width), generator=gen)
    return caps, ids, mask, z_t, feats


def _model(dtype, dropout_free=True):
    zf, g, v, sd2, _ = H.tiny_setup()
    m, _ = build(g, v, int(zf["seed"]), str(zf["profile"]), dtype)
    freeze_vit(m)
    if dropout_free:
        m.bert_geometry.hidden_dropout_prob = m.bert_geometry.attention_probs_dropout_prob = 0.0
    return m, g, sd2


def _oracle(w, z_t, feats, ids, mask, relu_mask, record=None):
    """(B, Bt) logits of the composed oracle: query i's caption / z_t expanded to the Bt candidates (blip_stage2.py:80-92), cls_head on the
    linear piece `relu_mask` (rows i * Bt + j) selects.  record[(i, layer, branch)] = the retained cross-attention probabilities."""
    from oracle import cir_oracle as O
    b, bt = z_t.shape[0], feats.shape[0]
    rows = []
    for i in range(b):
        def drop(kind, layer, br, x, i=i):
            if record is not None and kind == "cross_attn":
                x.retain_grad()
                record[(i, layer, br)] = x
            return x
        hid = O.nlvr_forward(w, ids[i:i + 1].expand(bt, -1), mask[i:i + 1].expand(bt, -1), z_t[i:i + 1].expand(bt, -1, -1), feats, drop=drop)
        y = F.linear(hid, w["cls_head.0.weight"], w["cls_head.0.bias"]) * relu_mask[i * bt:(i + 1) * bt].to(hid.dtype)
        rows.append(F.linear(y, w["cls_head.2.weight"], w["cls_head.2.bias"])[:, 0])
    return torch.stack(rows)


def _weights(sd2, trainable=True):
    w = {k: t.clone().float() for k, t in sd2.items()}
    keys = [k for k in w if k.startswith(("text_encoder.", "cls_head.")) and w[k].is_floating_point()]
    if trainable:
        for k in keys:
            w[k].requires_grad_(True)
    return w, keys


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_maps_match_oracle_autograd_and_gradcam_matches_maps(cuda, dtype):
    from candidate_reranking_cir_amd.train import model_trainer
    m, g, sd2 = _model(dtype)
    caps, ids, mask, z_t, feats = _inputs(g)
    m.eval()
    # the ReLU piece of this pass: the model's own trainer, run once by hand (the maps' pass repeats it bit for bit)
    tr = model_trainer(m, 0.0, 0.0, 0, cuda)
    logits0 = tr.forward(z_t.cuda(), feats.cuda(), ids.cuda(), mask.cuda()).clone()
    relu_mask = tr.head_mask().cpu()
    assert relu_mask.shape[0] == B_N * BT_N
    maps = m.cross_attention_maps(z_t.cuda(), feats.cuda(), caps, LAYERS)
    assert m.training is False and m._trainer is tr
    assert torch.equal(maps.logits, logits0), "the maps' logits are not the pass's own"
    l, n, h = ids.shape[1], feats.shape[1], g.num_attention_heads
    assert sorted(maps.probs) == sorted(maps.grads) == list(LAYERS)
    w, _ = _weights(sd2, trainable=False)
    record = {}
    feats_r = feats.clone().requires_grad_(True)                    # (something must require a gradient for the graph to exist)
    ref_logits = _oracle(w, z_t, feats_r, ids, mask, relu_mask, record)
    ref_logits.sum().backward()
    e_log = (maps.logits.cpu() - ref_logits.detach()).abs().max().item()
    assert e_log < 0.1 * ref_logits.std().item()
    worst = {"probs": 0.0, "grads": 0.0}
    for layer in LAYERS:
        p, gr = maps.probs[layer], maps.grads[layer]
        assert p.shape == gr.shape == (2, B_N, BT_N, h, l, n) and p.dtype == gr.dtype == torch.float32
        for t in (p, gr):                                           # views of the kernel's (2 Bt, H, B L, ldk) output, not copies
            assert t._is_view() and t._base.shape == (2 * BT_N, h, B_N * l, (n + 3) // 4 * 4)
        assert float((p.sum(-1) - 1).abs().max()) < 1e-4
        for br in (0, 1):
            rp = torch.stack([record[(i, layer, br)].detach() for i in range(B_N)])                  # (B, Bt, H, L, N)
            rg = torch.stack([record[(i, layer, br)].grad for i in range(B_N)])
            e_p = ((p[br].cpu() - rp).norm() / rp.norm()).item()
            e_g = ((gr[br].cpu() - rg).norm() / rg.norm()).item()
            print(f"\n[maps {dtype} layer {layer} branch {br}] probs rel L2 {e_p:.3e}  grads rel L2 {e_g:.3e}")
            worst = {"probs": max(worst["probs"], e_p), "grads": max(worst["grads"], e_g)}
            assert e_p < GRAD_REL[dtype] and e_g < GRAD_REL[dtype], (layer, br, e_p, e_g)
    print(f"\n[maps {dtype}] logits {e_log:.3e}; worst probs {worst['probs']:.3e}, worst grads {worst['grads']:.3e} (cap {GRAD_REL[dtype]})")
    # ---- Grad-CAM against the head mean formed in float64 from the maps' own tensors
    for layer in LAYERS:
        cam = m.gradcam(z_t.cuda(), feats.cuda(), caps, layer)
        assert cam.shape == (2, B_N, BT_N, l, n) and cam.dtype == torch.float32
        ref = (maps.probs[layer].double() * maps.grads[layer].double().clamp_min(0)).mean(3)
        # (H + 3) u: the kernel's fused sums, dmul, 1 / H;  u more: the fp32 rounding of the products a separate evaluation would make
        bnd = (h + 3) * U * ref + U * ref + 2.0 ** -149
        err = (cam.double() - ref).abs()
        print(f"[gradcam {dtype} layer {layer}] largest error / bound {float((err / bnd).max()):.3f}; max cam {float(ref.max()):.3e}")
        assert bool((err <= bnd).all())
        assert float(ref.max()) > 0
    with pytest.raises(TypeError):
        m.gradcam(z_t.cuda(), feats.cuda(), caps)                   # `layer` has no default
    with pytest.raises(ValueError):
        m.cross_attention_maps(z_t.cuda(), feats.cuda(), caps, (8,))
    only = m.cross_attention_maps(z_t.cuda(), feats.cuda(), caps, (7,), grads=False)
    assert only.grads is None and torch.equal(only.probs[7], maps.probs[7])


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_rectangular_training_step_matches_oracle_autograd(cuda, dtype):
    """B = 2 queries x Bt = 3 targets through fusion_train: logits, every parameter gradient and the gradient of the target tokens."""
    from candidate_reranking_cir_amd.train import fusion_train
    m, g, sd2 = _model(dtype)
    caps, ids, mask, z_t, feats = _inputs(g)
    m.train()
    f_dev = feats.cuda().requires_grad_(True)
    logits = fusion_train(m, z_t.cuda(), f_dev, ids.cuda(), mask.cuda(), 0.0, 0.0)
    assert logits.shape == (B_N, BT_N)
    dl = torch.randn((B_N, BT_N), generator=torch.Generator().manual_seed(4))
    (logits * dl.cuda()).sum().backward()
    tr = m._trainer
    assert tr.head_mask().shape[0] == B_N * BT_N
    w, keys = _weights(sd2)
    f_ref = feats.clone().requires_grad_(True)
    ref_logits = _oracle(w, z_t, f_ref, ids, mask, tr.head_mask().cpu())
    (ref_logits * dl).sum().backward()
    e_log = (logits.detach().cpu() - ref_logits.detach()).abs().max().item()
    params = dict(m.named_parameters())
    ref = {k: w[k].grad for k in keys if w[k].grad is not None}
    assert sorted(ref) == sorted(k for k, p in params.items() if p.grad is not None)
    gmax = max(t.norm().item() for t in ref.values())
    worst = (0.0, "")
    for k, r in ref.items():
        got = params[k].grad.cpu().view_as(r)
        if r.norm().item() < 1e-6 * gmax:
            assert got.norm().item() < 1e-3 * gmax, k
            continue
        e = ((got - r).norm() / r.norm()).item()
        worst = max(worst, (e, k))
        assert e < GRAD_REL[dtype], (k, e)
    assert f_dev.grad is not None and f_dev.grad.shape == feats.shape
    e_f = ((f_dev.grad.cpu() - f_ref.grad).norm() / f_ref.grad.norm()).item()
    print(f"\n[rectangular 2 x 3, {dtype}] logits {e_log:.3e} (sigma {ref_logits.std().item():.3f})  worst grad rel {worst[0]:.3e} ({worst[1]})  dfeats rel {e_f:.3e}")
    assert e_log < 0.1 * ref_logits.std().item()
    assert e_f < GRAD_REL[dtype]
    m.eval()


def _training_run(cuda, sequence):
    """A fresh fp16 tiny model (dropout at the config's probabilities), AdamW, and `sequence` of "step" | "fwd" | "bwd" | "opt" | "explain" ->
    (parameters, moments)."""
    from candidate_reranking_cir_amd.train import AdamW
    m, g, _ = _model(HF, dropout_free=False)
    caps, ids, mask, z_t, feats = _inputs(g, b=3, bt=3, seed=21)
    z_t, feats = z_t.cuda(), feats.cuda()
    gt = torch.arange(3, device=cuda)
    m.train()
    ps = [p for p in m.parameters() if p.requires_grad]
    opt = AdamW(ps, lr=1e-3, weight_decay=0.05, model=m)
    loss = None
    for what in sequence:
        if what in ("step", "fwd"):
            opt.zero_grad()
            loss = F.cross_entropy(m.img_txt_fusion(z_t, feats, caps), gt)
        if what in ("step", "bwd"):
            loss.backward()
        if what in ("step", "opt"):
            opt.step()
        if what == "explain":
            tr, slab = m._trainer, m._trainer.slab
            before = (tr.sv, tr.step_no, tr.generation, tr.consumed, tr.grads_finite, tr.grad_scale, slab.checked, slab.gflat, tr.p_hidden, tr.p_attn,
                      [None if p.grad is None else p.grad.data_ptr() for p in ps])
            maps = m.cross_attention_maps(z_t, feats[:2], caps, (3, 7))
            cam = m.gradcam(z_t, feats[:2], caps, 0)
            assert maps.logits.shape == (3, 2) and cam.shape[:3] == (2, 3, 2) and m.training
            after = (tr.sv, tr.step_no, tr.generation, tr.consumed, tr.grads_finite, tr.grad_scale, slab.checked, slab.gflat, tr.p_hidden, tr.p_attn,
                     [None if p.grad is None else p.grad.data_ptr() for p in ps])
            assert m._trainer is tr and tr.slab is slab and all(a is b_ or a == b_ for a, b_ in zip(before, after))
    assert opt.skipped_steps == 0
    live = [p for p in ps if id(p) in opt.m]
    assert len(live) > 300
    return [p.detach().clone() for p in ps], [opt.m[id(p)].clone() for p in live], [opt.v[id(p)].clone() for p in live]


def test_explaining_does_not_disturb_a_training_run(cuda):
    from candidate_reranking_cir_amd.train import set_deterministic
    set_deterministic(True)
    try:
        plain = _training_run(cuda, ("step", "step"))
        between = _training_run(cuda, ("step", "explain", "step"))
        inside = _training_run(cuda, ("fwd", "bwd", "explain", "opt", "step"))
    finally:
        set_deterministic(False)
    for name, other in (("step, explain, step", between), ("forward, backward, explain, optimizer.step(), step", inside)):
        for kind, a, b_ in zip(("parameters", "exp_avg", "exp_avg_sq"), plain, other):
            assert all(torch.equal(x, y) for x, y in zip(a, b_)), f"{name}: {kind} differ from step, step"


def test_explaining_between_a_forward_and_its_backward_raises(cuda):
    from candidate_reranking_cir_amd.train import set_deterministic
    set_deterministic(True)
    try:
        grads = []
        for attempt in (True, False):
            m, g, _ = _model(HF, dropout_free=False)
            caps, ids, mask, z_t, feats = _inputs(g, b=3, bt=3, seed=21)
            m.train()
            loss = F.cross_entropy(m.img_txt_fusion(z_t.cuda(), feats.cuda(), caps), torch.arange(3, device=cuda))
            if attempt:
                with pytest.raises(RuntimeError, match="between a training-mode forward and its backward"):
                    m.gradcam(z_t.cuda(), feats.cuda(), caps, 7)
                with pytest.raises(RuntimeError, match="between a training-mode forward and its backward"):
                    m.cross_attention_maps(z_t.cuda(), feats.cuda(), caps, (7,))
            loss.backward()
            grads.append([p.grad.clone() for p in m.parameters() if p.grad is not None])
    finally:
        set_deterministic(False)
    assert len(grads[0]) == len(grads[1]) > 300 and all(torch.equal(a, b_) for a, b_ in zip(*grads))
