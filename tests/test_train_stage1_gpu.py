"""Stage-I training step on a real MI355X: `BLIP_Retrieval.img_txt_fusion(..., train=True)` in .train() mode and its hand-written reverse
pass (candidate_reranking_cir_amd/train_stage1.py) against the REAL reference's gradients (tests/golden/train_s1*.npz, tools/
make_stage1_train_golden.py), the CPU oracle's autograd, and the reference loop's own forms (autocast + GradScaler, micro-batches,
AdamW).  Bounds are relative to each tensor's own gradient norm; measured values are printed with -s.  The contrastive head has no ReLU,
so the reference's gradients are compared directly with the same-piece bounds of tests/test_train_gpu.py."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests.test_train_stage1_cpu import fixture_inputs, oracle_logits

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16
GRAD_REL = {BF: 0.12, HF: 0.016}             # worst tensor: relative L2 error of the sampled entries / of the norm
GRAD_REL_MEAN = {BF: 0.03, HF: 0.004}        # norm-weighted mean over the tensors
TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, layer_norm_eps=1e-12, vocab_size=30524,
            max_position_embeddings=512, encoder_width=1024, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
TINY_VIT = dict(image_size=64, width=1024, depth=1, num_heads=16)      # ViT-L width: 1024-wide image tokens, hidden 128


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def build(g, v, seed, profile, dtype, precision=None):
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    _, sd1 = H.state_dicts(g, v, seed, profile)
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m1.load_state_dict(sd1, strict=True)
    m1 = m1.cuda().float()
    if precision is not None:
        m1.set_precision(precision)
    else:
        m1.set_compute_dtype(dtype)
    return m1, sd1


def grad_errors(named_grads, ref_grads, names, gmax):
    """(worst (error, name), norm-weighted mean) of per-tensor relative errors; analytically zero gradients get an absolute bound."""
    worst, num, den = (0.0, ""), 0.0, 0.0
    for n in names:
        got, ref = named_grads[n].double().flatten(), ref_grads[n].double().flatten()
        rn = ref.norm().item()
        if rn < 1e-6 * gmax:                                          # key biases: softmax is shift-invariant
            assert got.norm().item() < 1e-3 * gmax, n
            continue
        e = (got - ref).norm().item() / rn
        if e > worst[0]:
            worst = (e, n)
        num += e * rn
        den += rn
    return worst, num / den


def tokens(caps, l=None):
    enc = synthetic.HashTokenizer()(list(caps))
    ids, mask = enc.input_ids, enc.attention_mask
    if l is not None and ids.shape[1] < l:
        pad = l - ids.shape[1]
        ids, mask = F.pad(ids, (0, pad)), F.pad(mask, (0, pad))
    return {"input_ids": ids, "attention_mask": mask}


# ------------------------------------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("fixture", ["train_s1", "train_s1_577"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_training_step_matches_reference(cuda, dtype, fixture):
    z = H.load(fixture + ".npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    m1, _ = build(g, v, int(z["seed"]), str(z["profile"]), dtype)
    ref, tgt = fixture_inputs(z)
    m1.train()
    caps = [str(c) for c in z["caps"]]
    b = len(caps)
    logits = m1.img_txt_fusion(ref.cuda(), tgt.cuda(), caps, train=True)
    assert logits.shape == (b, b) and logits.dtype == torch.float32 and logits.requires_grad
    loss = F.cross_entropy(logits, torch.arange(b, device=cuda))
    loss.backward()
    params = dict(m1.named_parameters())
    names = [str(n) for n in z["names"]]
    assert sorted(names) == sorted(n for n, p in params.items() if p.grad is not None), "set of parameters that received a gradient"
    gmax = float(z["norms"].max())
    worst, num, den = (0.0, ""), 0.0, 0.0
    for i, n in enumerate(names):
        gq = params[n].grad.detach().flatten()
        ref_norm = float(z["norms"][i])
        if ref_norm < 1e-6 * gmax:                                    # key biases: absolute bound against the largest gradient
            assert gq.double().norm().item() < 1e-3 * gmax, n
            continue
        got = gq[torch.from_numpy(H.grad_sample_index(gq.numel())).cuda()].cpu().numpy()
        rms = ref_norm / np.sqrt(gq.numel())
        e = max(float(np.sqrt(np.mean((got - z["samples"][i]) ** 2)) / rms), abs(gq.double().norm().item() - ref_norm) / ref_norm)
        if e > worst[0]:
            worst = (e, n)
        num += e * ref_norm
        den += ref_norm
    full = {}
    for key in z.files:
        if key.startswith("full__"):
            full[key[6:]] = np.linalg.norm(params[key[6:]].grad.cpu().numpy() - z[key]) / np.linalg.norm(z[key])
    e_log = np.abs(logits.detach().cpu().numpy() - z["logits"]).max()
    print(f"\n[{fixture} {dtype}] logits {e_log:.3e} (sigma {z['logits'].std():.3f})  loss {loss.item():.5f} vs {float(z['loss']):.5f}  "
          f"worst grad rel {worst[0]:.3e} ({worst[1]})  norm-weighted mean {num / den:.3e}  full {({k: round(float(x), 5) for k, x in full.items()})}")
    assert e_log < (0.05 if dtype == BF else 0.01) and abs(loss.item() - float(z["loss"])) < (0.02 if dtype == BF else 0.004)
    assert full["temp"] < GRAD_REL[dtype] and all(x < GRAD_REL[dtype] for x in full.values())
    assert worst[0] < GRAD_REL[dtype] and num / den < GRAD_REL_MEAN[dtype]


# ------------------------------------------------------------------------------------------------------------------ 2. tiny vs oracle
def _tiny(dtype, p_drop=0.0, precision=None):
    g, v = H.geometry(dict(TINY, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop), TINY_VIT)
    m1, sd1 = build(g, v, 7, "test", dtype, precision)
    caps = [synthetic.caption_text(900 + i, n) for i, n in enumerate((5, 11, 3))]
    gen = torch.Generator().manual_seed(33)
    ref = torch.randn((3, 17, 1024), generator=gen)
    tgt = F.normalize(torch.randn((5, 256), generator=gen), dim=-1)                      # Bt != B
    wl = torch.randn((3, 5), generator=gen)                                             # a loss with every logit in play
    return g, m1, sd1, caps, ref, tgt, wl


def _oracle_grads(sd1, names, caps, ref, tgt, wl, dtype, drop=None):
    w = {k: t.double() for k, t in sd1.items()}
    for n in names:
        w[n].requires_grad_(True)
    tok = tokens(caps)
    ids = tok["input_ids"].clone()
    ids[:, 0] = 30523
    lo = oracle_logits(w, ids, tok["attention_mask"], ref.to(dtype).double(), tgt.double(), drop=drop)
    (lo * wl.double()).sum().backward()
    return lo.detach(), {n: w[n].grad for n in names}


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_tiny_geometry_against_oracle_autograd(cuda, dtype):
    g, m1, sd1, caps, ref, tgt, wl = _tiny(dtype)
    assert g.encoder_width == 1024 != g.hidden_size
    m1.train()
    logits = m1.img_txt_fusion(ref.cuda(), tgt.cuda(), caps)
    (logits * wl.cuda()).sum().backward()
    names = [n for n, p in m1.named_parameters() if p.grad is not None]
    assert len(names) == 26 * g.num_hidden_layers + 7
    o_logits, o_grads = _oracle_grads(sd1, names, caps, ref, tgt, wl, dtype)
    got = {n: p.grad.cpu() for n, p in m1.named_parameters() if p.grad is not None}
    worst, mean = grad_errors(got, o_grads, names, max(t.norm().item() for t in o_grads.values()))
    e_log = (logits.detach().cpu().double() - o_logits).abs().max().item()
    print(f"\n[tiny {dtype}] logits {e_log:.3e}  worst grad rel {worst[0]:.3e} ({worst[1]})  mean {mean:.3e}")
    assert e_log < (0.1 if dtype == BF else 0.02)
    assert worst[0] < GRAD_REL[dtype] and mean < GRAD_REL_MEAN[dtype]


# ------------------------------------------------------------------------------------------------------------------ 3. dropout
def test_dropout_masks_seed_and_oracle(cuda):
    from tests.test_train_med_gpu import _hooks
    g, m1, sd1, caps, ref, tgt, wl = _tiny(HF, p_drop=0.1)
    m1.train()
    r, t, w = ref.cuda(), tgt.cuda(), wl.cuda()

    def step(seed):
        torch.manual_seed(seed)
        m1.zero_grad(set_to_none=True)
        lo = m1.img_txt_fusion(r, t, caps)
        (lo * w).sum().backward()
        return lo.detach().clone(), {n: p.grad.detach().clone() for n, p in m1.named_parameters() if p.grad is not None}, m1._trainer.last_seed

    a, ga, sa = step(5)
    b, gb, sb = step(5)
    c, _, sc = step(6)
    assert sa == sb != sc and torch.equal(a, b) and not torch.equal(a, c)
    for n in ga:
        assert torch.allclose(ga[n], gb[n], rtol=1e-5, atol=1e-6 * ga[n].abs().max().item()), n      # up to the fp32 atomic adds' order
    # the kernels' own masks, regenerated on the host, handed to the oracle
    q_n, l = tokens(caps)["input_ids"].shape
    drop, kept = _hooks(sa, q_n, l, ref.shape[1], g.hidden_size, g.num_attention_heads, 0.1, 0.1)
    names = list(ga)
    o_logits, o_grads = _oracle_grads(sd1, names, caps, ref, tgt, wl, HF, drop=drop)
    worst, mean = grad_errors({n: x.cpu() for n, x in ga.items()}, o_grads, names, max(x.norm().item() for x in o_grads.values()))
    e_log = (a.cpu().double() - o_logits).abs().max().item()
    print(f"\n[dropout 0.1 fp16] logits {e_log:.3e}  worst grad rel {worst[0]:.3e} ({worst[1]})  mean {mean:.3e}  kept {np.mean(kept):.3f}")
    assert abs(np.mean(kept) - 0.9) < 0.03 and e_log < 0.02 and worst[0] < GRAD_REL[HF] and mean < GRAD_REL_MEAN[HF]


# ------------------------------------------------------------------------------------------------------------------ 4. reference batch
def test_reference_batch_rows_are_independent(cuda):
    """B = 1024, L = 40 ragged, N = 577: the first 8 rows / columns of the logits are bit-equal to a B = 8 run, and with dlogits supported
    on that block the gradients agree up to the order of the fp32 atomic adds."""
    g, v = H.geometry(dict(H.FULL_BERT, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), dict(image_size=384, width=768, depth=1, num_heads=12))
    m1, _ = build(g, v, 31, "test", HF)
    m1.train()
    big = 1024
    caps = [synthetic.caption_text(5000 + i, 5 + (i * 7) % 34) for i in range(big)]
    caps[3] = synthetic.caption_text(4999, 38)                                       # L = 40
    tok = tokens(caps)
    assert tok["input_ids"].shape[1] == 40
    gen = torch.Generator().manual_seed(1024)
    ref = torch.randn((big, 577, 768), generator=gen).cuda()
    tgt = F.normalize(torch.randn((big, 256), generator=gen), dim=-1).cuda()
    d8 = torch.randn((8, 8), generator=gen).cuda()
    logits = m1.img_txt_fusion(ref, tgt, tok)
    dl = torch.zeros((big, big), device=cuda)
    dl[:8, :8] = d8
    logits.backward(dl)
    g_big = {n: p.grad.detach().clone() for n, p in m1.named_parameters() if p.grad is not None}
    block = logits.detach()[:8, :8].clone()
    del logits, dl
    m1.zero_grad(set_to_none=True)
    small = {k: x[:8] for k, x in tok.items()}
    l8 = m1.img_txt_fusion(ref[:8].contiguous(), tgt[:8].contiguous(), small)
    l8.backward(d8)
    assert torch.equal(l8.detach(), block)
    worst, gmax = (0.0, ""), max(x.norm().item() for x in g_big.values())
    for n, p in m1.named_parameters():
        if p.grad is None:
            continue
        diff = (p.grad - g_big[n]).norm().item()
        if n.endswith(".self.key.bias"):                                             # analytically zero: absolute bound
            assert diff < 1e-6 * gmax, n
            continue
        e = diff / max(g_big[n].norm().item(), 1e-30)
        if e > worst[0]:
            worst = (e, n)
    print(f"\n[B 1024 vs 8] worst gradient difference {worst[0]:.3e} ({worst[1]})")
    assert worst[0] < 1e-4


# ------------------------------------------------------------------------------------------------------------------ 5. fp16 loop
def test_fp16_loop_at_reference_geometry(cuda):
    from candidate_reranking_cir_amd import train
    g, v = H.geometry(dict(H.FULL_BERT, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), dict(image_size=384, width=768, depth=1, num_heads=12))
    m1, _ = build(g, v, 41, "test", HF)
    m1.train()
    b = 64
    caps = [synthetic.caption_text(7000 + i, 4 + i % 20) for i in range(b)]
    gen = torch.Generator().manual_seed(64)
    ref = torch.randn((b, 577, 768), generator=gen).cuda()
    tgt = F.normalize(torch.randn((b, 256), generator=gen), dim=-1).cuda()
    params = [p for p in m1.parameters() if p.requires_grad]
    opt = train.AdamW(params, lr=2e-5, weight_decay=0.05, model=m1)
    temp0 = float(m1.temp.detach())
    losses = []
    for _ in range(8):
        torch.manual_seed(123)                                                       # the same dropout draw every step: the loss moves by the updates
        opt.zero_grad()
        loss = F.cross_entropy(m1.img_txt_fusion(ref, tgt, caps), torch.arange(b, device=cuda))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"\n[fp16 loop B 64] losses {[round(x, 4) for x in losses]}  temp {temp0:.6f} -> {float(m1.temp.detach()):.6f}")
    assert opt.skipped_steps == 0 and opt.t == 8
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and float(m1.temp.detach()) != temp0


# ------------------------------------------------------------------------------------------------------------------ 6. reference loop form
def test_reference_loop_autocast_gradscaler_and_micro_batches(cuda):
    from candidate_reranking_cir_amd import train
    g, m1, sd1, caps, ref, tgt, wl = _tiny(HF, p_drop=0.1)
    m1.train()
    r, t = ref.cuda(), tgt[:3].cuda()
    gt = torch.arange(3, device=cuda)
    opt = torch.optim.AdamW([p for p in m1.parameters() if p.requires_grad], lr=2e-5, weight_decay=0.05)
    scaler = torch.cuda.amp.GradScaler()
    w0 = m1.text_proj.weight.detach().clone()
    for _ in range(2):                                                               # stage1_train.py:170-192
        opt.zero_grad()
        with torch.cuda.amp.autocast():
            logits = m1.img_txt_fusion(r, t, caps, train=True)
            loss = torch.nn.CrossEntropyLoss()(logits, gt)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    assert torch.isfinite(loss) and not torch.equal(w0, m1.text_proj.weight)
    # two micro-batches accumulate to the sum of their gradients, and train.AdamW keeps its one flat launch
    trained = [p for p in m1.parameters() if p.requires_grad]
    single = []
    for s in (8, 9):
        m1.zero_grad(set_to_none=True)
        torch.manual_seed(s)
        F.cross_entropy(m1.img_txt_fusion(r, t, caps), gt).backward()
        single.append([None if p.grad is None else p.grad.clone() for p in trained])
    m1.zero_grad(set_to_none=True)
    for s in (8, 9):
        torch.manual_seed(s)
        F.cross_entropy(m1.img_txt_fusion(r, t, caps), gt).backward()
    for p, a, b in zip(trained, *single):
        if a is None:
            assert p.grad is None
            continue
        assert torch.allclose(p.grad, a + b, rtol=1e-5, atol=1e-6 * (a.abs().max().item() + b.abs().max().item())), p.shape
    assert len({p.grad.untyped_storage().data_ptr() for p in trained if p.grad is not None}) == 1      # one flat gradient buffer
    opt2 = train.AdamW([p for p in trained if p.grad is not None], lr=2e-5, weight_decay=0.05, model=m1)
    grp = [p for p in trained if p.grad is not None]
    plan = opt2._plan(grp)
    assert plan is not None and opt2._grads_match(grp, plan) is not None                                  # the flat path
    opt2.step()
    assert opt2.t == 1


# ------------------------------------------------------------------------------------------------------------------ 7. modes and guards
def test_modes_and_guards(cuda):
    from candidate_reranking_cir_amd import ops, train_ops as T
    g, m1, sd1, caps, ref, tgt, wl = _tiny(HF, p_drop=0.1)
    r, t = ref.cuda(), tgt.cuda()
    tok = tokens(caps)
    ids = tok["input_ids"].cuda().clone()
    ids[:, 0] = 30523
    mask = tok["attention_mask"].cuda()

    def head(h):
        heads = m1.engines()[2]
        return T.contrastive_fwd(ops.linear_f32(h[:, 0, :], heads["tw"], heads["tb"]), t, heads["temp"])[2]
    m1.eval()
    feat0 = m1.img_txt_fusion(r, t, caps, train=False)
    raw0 = m1.img_txt_fusion(r, t, caps, train=False, return_raw=True).last_hidden_state.clone()
    e = m1.img_txt_fusion(r, t, caps)
    assert not e.requires_grad and torch.equal(e, head(m1.z_t(r, ids, mask).last_hidden_state))
    m1.train()
    with torch.no_grad():
        torch.manual_seed(3)
        a = m1.img_txt_fusion(r, t, caps)
        torch.manual_seed(3)
        assert torch.equal(a, head(m1.z_t(r, ids, mask).last_hidden_state))
    # a training step leaves train=False and z_t as they were
    F.cross_entropy(m1.img_txt_fusion(r, t[:3], caps), torch.arange(3, device=cuda)).backward()
    m1.eval()
    assert torch.equal(m1.img_txt_fusion(r, t, caps, train=False), feat0)
    assert torch.equal(m1.img_txt_fusion(r, t, caps, train=False, return_raw=True).last_hidden_state, raw0)
    m1.train()
    with pytest.raises(NotImplementedError, match="blip-img-tune"):
        m1.img_txt_fusion(r.clone().requires_grad_(True), t, caps)
    with pytest.raises(NotImplementedError, match="blip-img-tune"):
        m1.img_txt_fusion(r, t.clone().requires_grad_(True), caps)
    l1 = m1.img_txt_fusion(r, t, caps)
    l2 = m1.img_txt_fusion(r, t, caps)
    with pytest.raises(RuntimeError, match="another training-mode forward"):
        l1.sum().backward()
    l2.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        l2.sum().backward()
    m1.eval()


# ------------------------------------------------------------------------------------------------------------------ 8. text32
def test_text32_model_trains_like_f16(cuda):
    out = []
    for prec in ("f16", "text32"):
        g, m1, sd1, caps, ref, tgt, wl = _tiny(HF, precision=prec)
        m1.train()
        lo = m1.img_txt_fusion(ref.cuda(), tgt.cuda(), caps)
        (lo * wl.cuda()).sum().backward()
        assert m1._trainer.dtype == HF
        out.append((lo.detach(), {n: p.grad.detach().clone() for n, p in m1.named_parameters() if p.grad is not None}))
    assert torch.equal(out[0][0], out[1][0]) and sorted(out[0][1]) == sorted(out[1][1])
    for n, x in out[0][1].items():
        assert torch.allclose(x, out[1][1][n], rtol=1e-5, atol=1e-6 * x.abs().max().item()), n


# ------------------------------------------------------------------------------------------------------------------ 9. staleness
def test_parameter_writes_reach_the_next_forward(cuda):
    from candidate_reranking_cir_amd import train
    g, m1, sd1, caps, ref, tgt, wl = _tiny(HF)
    r, t = ref.cuda(), tgt.cuda()
    fresh = lambda: _tiny(HF)[1]
    m1.train()

    def both(m):
        m.train()
        lo = m.img_txt_fusion(r, t, caps)
        lo.sum().backward()
        m.zero_grad(set_to_none=True)
        m.eval()
        ev = m.img_txt_fusion(r, t, caps)
        m.train()
        return lo.detach(), ev

    both(m1)                                                                          # the slab and engines exist
    opt = train.AdamW([p for p in m1.parameters() if p.requires_grad], lr=1e-3, model=m1)
    m1.img_txt_fusion(r, t, caps).sum().backward()
    opt.step()
    m1.zero_grad(set_to_none=True)
    twin = fresh()
    twin.load_state_dict(m1.state_dict())
    a, b = both(m1), both(twin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                       # AdamW.step
    sd = {k: v.clone() for k, v in m1.state_dict().items()}
    for k in ("temp", "text_proj.weight", "text_encoder.encoder.layer.1.output.dense.weight"):
        sd[k] = sd[k] * 1.25
    m1.load_state_dict(sd)
    twin.load_state_dict(sd)
    a, b = both(m1), both(twin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                       # load_state_dict
    for name in ("temp", "text_proj.weight", "text_encoder.encoder.layer.0.attention.self.query.weight"):
        before = both(m1)
        p = dict(m1.named_parameters())[name]
        p.data.copy_(p.data * 0.5 + 0.01)
        m1.invalidate_packed_weights()
        q = dict(twin.named_parameters())[name]
        q.data.copy_(q.data * 0.5 + 0.01)
        twin.invalidate_packed_weights()
        a, b = both(m1), both(twin)
        assert not torch.equal(a[0], before[0]) and not torch.equal(a[1], before[1]), name
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        with torch.no_grad():                                                         # an in-place torch op: seen without invalidation
            p.mul_(1.5)
            q.mul_(1.5)
        a, b = both(m1), both(twin)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


# ------------------------------------------------------------------------------------------------------------------ 10. head kernels
def test_head_kernels_against_fp64(cuda):
    from candidate_reranking_cir_amd import train_ops as T
    gen = torch.Generator().manual_seed(99)
    b, bt, e, d, l = 37, 53, 256, 96, 3
    p = torch.randn((b, e), generator=gen)
    tgt = F.normalize(torch.randn((bt, e), generator=gen), dim=-1)
    temp = torch.tensor([0.07])
    x = torch.randn((b, l * d), generator=gen)                                        # CLS rows at stride l * d
    w = torch.randn((e, d), generator=gen) * 0.05
    dl = torch.randn((b, bt), generator=gen)
    pd, xd, wd, td = (t.double().requires_grad_(True) for t in (p, x[:, :d].contiguous(), w, temp))
    ref_logits = F.normalize(pd, dim=-1) @ tgt.double().t() / td
    ref_logits.backward(dl.double())
    # the projection's adjoint: p = x W^T + bias -> dx = dp W, dW = dp^T x, db = sum dp
    pc, xc, wc = p.cuda(), x.cuda(), w.cuda()
    runs = []
    for _ in range(2):
        p_hat, inv, logits = T.contrastive_fwd(pc, tgt.cuda(), temp.cuda())
        dtemp = torch.full((1,), 123.0, device=cuda)
        dx = torch.full((b, l * d), 7.0, device=cuda)
        dw, db = torch.full((e, d), 5.0, device=cuda), torch.full((e,), 5.0, device=cuda)
        dp = T.contrastive_bwd(dl.cuda(), tgt.cuda(), temp.cuda(), p_hat, inv, dtemp, x=xc[:, :d], w=wc, dx=dx[:, :d], dw=dw, db=db)
        runs.append([t.cpu() for t in (p_hat, inv, logits, dp, dtemp, dx, dw, db)])
    for u, v in zip(*runs):
        assert torch.equal(u, v)                                                      # bitwise reproducible
    p_hat, inv, logits, dp, dtemp, dx, dw, db = runs[0]
    rel = lambda got, ref: ((got.double() - ref).norm() / ref.norm()).item()
    assert rel(p_hat, F.normalize(p.double(), dim=-1)) < 1e-6 and rel(inv, 1 / p.double().norm(dim=-1)) < 1e-6
    assert rel(logits, ref_logits.detach()) < 1e-6
    assert rel(dp, pd.grad) < 1e-5 and abs(dtemp.item() - td.grad.item()) < 1e-5 * abs(td.grad.item())
    dpd = dp.double()
    assert rel(dx[:, :d], dpd @ w.double()) < 1e-5 and rel(dw, dpd.t() @ x[:, :d].double()) < 1e-5 and rel(db, dpd.sum(0)) < 1e-5
    assert torch.all(dx[:, d:] == 7.0)                                                # only the CLS rows are written
