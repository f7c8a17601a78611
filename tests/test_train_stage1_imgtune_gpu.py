"""Stage-I training with a trainable image encoder (`BLIP_Retrieval.set_image_tuning()`, stage1_train.py --blip-img-tune) on a real
MI355X: one step of the REAL reference (tests/golden/train_s1_imgtune*.npz, tools/make_stage1_imgtune_golden.py) through img_embed ->
img_txt_fusion -> backward, the two input gradients of `MedTrainer` against the CPU oracle's autograd, what the switch must leave alone,
the reference's loop (autocast, GradScaler, blip_bs mini-batches, AdamW), the guards, and the three new entry points against float64.

Measured on the MI355X (worst tensor | norm-weighted mean of the per-tensor relative errors; printed with -s), asserted at about 2 x:

    one step of the reference          fp16 worst   fp16 mean    bf16 worst   bf16 mean
      train_s1_imgtune      (N 17)     2.41e-3      1.20e-3      2.21e-2      1.22e-2
      train_s1_imgtune_577  (N 577)    6.38e-3      2.63e-3      4.62e-2      2.07e-2
    (whole batch and mini-batches of 2 give the same figures; text side alone: 2.06e-3 / 6.38e-3 fp16, 2.21e-2 / 4.62e-2 bf16 worst)
    input gradients vs oracle          d ref_tokens (fp16 | bf16)             d target (fp16 | bf16)
      all four shapes, worst           5.38e-4 | 4.17e-3                      5.02e-5 | 4.08e-4

The 319 text-side tensors are also held to the bounds tests/test_train_stage1_gpu.py holds them to on train_s1 / train_s1_577
(worst 0.016 / 0.12, mean 0.004 / 0.03 for fp16 / bf16): the image side does not loosen them."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16
TEXT_REL, TEXT_REL_MEAN = {BF: 0.12, HF: 0.016}, {BF: 0.03, HF: 0.004}       # tests/test_train_stage1_gpu.py: GRAD_REL, GRAD_REL_MEAN
ALL_REL = {"train_s1_imgtune": {HF: 5e-3, BF: 4.4e-2}, "train_s1_imgtune_577": {HF: 1.3e-2, BF: 9.2e-2}}          # all tensors, worst: 2 x measured
ALL_REL_MEAN = {"train_s1_imgtune": {HF: 2.4e-3, BF: 2.5e-2}, "train_s1_imgtune_577": {HF: 5.3e-3, BF: 4.1e-2}}     # all tensors, mean: 2 x measured
DIN_REL = {"ref": {HF: 1.1e-3, BF: 8.4e-3}, "target": {HF: 1.0e-4, BF: 8.2e-4}}                                        # input gradients: 2 x measured
TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, layer_norm_eps=1e-12, vocab_size=30524,
            max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
U = 2.0 ** -24                                                                # unit round-off of fp32 = eps32 / 2


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture
def deterministic():
    from candidate_reranking_cir_amd import train
    assert train.deterministic() is False
    train.set_deterministic(True)
    yield
    train.set_deterministic(False)


def build(g, v, seed, profile, dtype, tuning=True):
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    _, sd1 = H.state_dicts(g, v, seed, profile)
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m1.load_state_dict(sd1, strict=True)
    m1 = m1.cuda().float()
    m1.set_compute_dtype(dtype)
    return (m1.set_image_tuning() if tuning else m1), sd1


def tiny(dtype, width=768, image_size=64, depth=1, p_drop=0.0, tuning=True, seed=7):
    g, v = H.geometry(dict(TINY, encoder_width=width, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop),
                      dict(image_size=image_size, width=width, depth=depth, num_heads=width // 64))
    m1, sd1 = build(g, v, seed, "test", dtype, tuning)
    return g, v, m1, sd1


def grads_of(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def sampled_errors(params, z, names, gmax):
    """(worst (error, name), norm-weighted mean) of the per-tensor relative errors against a fixture, which keeps per tensor its norm and the
    64 entries of `grad_sample_index`: the error of a tensor is the larger of the samples' relative RMS error and the norm's relative error;
    analytically zero gradients (key biases: softmax is shift-invariant) get an absolute bound - `grad_errors` and the fixture test of
    tests/test_train_stage1_gpu.py, restated.  No tensor is left out."""
    index = {str(n): i for i, n in enumerate(z["names"])}
    worst, num, den = (0.0, ""), 0.0, 0.0
    for n in names:
        i = index[n]
        gq = params[n].grad.detach().flatten()
        ref_norm = float(z["norms"][i])
        if ref_norm < 1e-6 * gmax:
            assert gq.double().norm().item() < 1e-3 * gmax, n
            continue
        got = gq[torch.from_numpy(H.grad_sample_index(gq.numel())).cuda()].cpu().numpy()
        rms = ref_norm / np.sqrt(gq.numel())
        e = max(float(np.sqrt(np.mean((got - z["samples"][i]) ** 2)) / rms), abs(gq.double().norm().item() - ref_norm) / ref_norm)
        if e > worst[0]:
            worst = (e, n)
        num += e * ref_norm
        den += ref_norm
    return worst, num / den


def fixture_images(z, size):
    gen = torch.Generator().manual_seed(int(z["input_seed"]))
    b = z["input_ids"].shape[0]
    ri, ti = torch.randn((b, 3, size, size), generator=gen), torch.randn((b, 3, size, size), generator=gen)
    np.testing.assert_array_equal(ri[:, :, :2, :8].numpy(), z["ref_image_slice"])
    np.testing.assert_array_equal(ti[:, :, :2, :8].numpy(), z["tgt_image_slice"])
    return ri, ti


def embed(m, ri, ti, bs=None):
    """stage1_train.py:144-164: both sides through img_embed, whole or in `bs` mini-batches joined by torch.vstack."""
    if bs is None:
        return m.img_embed(ri), m.img_embed(ti, return_pool_and_normalized=True)[-1]
    ref = torch.vstack([m.img_embed(ri[i:i + bs]) for i in range(0, ri.shape[0], bs)])
    tgt = torch.vstack([m.img_embed(ti[i:i + bs], return_pool_and_normalized=True)[-1] for i in range(0, ti.shape[0], bs)])
    return ref, tgt


# ------------------------------------------------------------------------------------------------------------------ 1. the reference's step
@pytest.mark.parametrize("fixture", ["train_s1_imgtune", "train_s1_imgtune_577"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_tuned_step_matches_reference(cuda, dtype, fixture):
    z = H.load(fixture + ".npz")
    vit_cfg = json.loads(str(z["vit_cfg"]))
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), vit_cfg)
    m1, _ = build(g, v, int(z["seed"]), str(z["profile"]), dtype)
    assert m1.image_tuning and m1.vit_geometry.drop_path_rate == 0.0
    ri, ti = (t.cuda() for t in fixture_images(z, vit_cfg["image_size"]))
    m1.train()
    caps = [str(c) for c in z["caps"]]
    b = len(caps)
    names = [str(n) for n in z["names"]]
    text = [n for n in names if not n.startswith(("visual_encoder.", "vision_proj."))]
    assert len(text) == 319 and len(names) == {"train_s1_imgtune": 351, "train_s1_imgtune_577": 339}[fixture]
    gmax = float(z["norms"].max())
    for bs in (None, 2):
        m1.zero_grad(set_to_none=True)
        ref, tgt = embed(m1, ri, ti, bs)
        assert ref.requires_grad and tgt.requires_grad and ref.shape == (b, int(z["n_tok"]), 768) and tgt.shape == (b, 256)
        e_tok = (ref.detach()[:, :3, :16].cpu() - torch.from_numpy(z["tokens_slice"])).abs().max().item()
        e_pool = (tgt.detach()[:, :16].cpu() - torch.from_numpy(z["pooled_slice"])).abs().max().item()
        logits = m1.img_txt_fusion(ref, tgt, caps, train=True)
        assert logits.shape == (b, b) and logits.dtype == torch.float32 and logits.requires_grad
        loss = F.cross_entropy(logits, torch.arange(b, device=cuda))
        loss.backward()
        params = dict(m1.named_parameters())
        assert sorted(names) == sorted(n for n, p in params.items() if p.grad is not None), "set of parameters that received a gradient"
        worst, mean = sampled_errors(params, z, names, gmax)
        t_worst, t_mean = sampled_errors(params, z, text, gmax)
        full = {key[6:]: float(np.linalg.norm(params[key[6:]].grad.cpu().numpy() - z[key]) / np.linalg.norm(z[key])) for key in z.files if key.startswith("full__")}
        e_log = np.abs(logits.detach().cpu().numpy() - z["logits"]).max()
        print(f"\n[{fixture} {dtype} mini-batch {bs}] tokens {e_tok:.3e} pooled {e_pool:.3e} logits {e_log:.3e} (sigma {z['logits'].std():.3f})  loss {loss.item():.5f} vs "
              f"{float(z['loss']):.5f}  worst grad rel {worst[0]:.3e} ({worst[1]})  mean {mean:.3e}  text side worst {t_worst[0]:.3e} ({t_worst[1]}) mean "
              f"{t_mean:.3e}  full {({k: round(x, 5) for k, x in full.items()})}")
        # the forward slices (largest entry-wise difference; measured 1.53e-2 / 2.52e-3 tokens, 1.19e-3 / 1.17e-4 pooled for bf16 / fp16: 2 x)
        assert e_tok < (3.1e-2 if dtype == BF else 5e-3) and e_pool < (2.4e-3 if dtype == BF else 2.4e-4)
        assert e_log < (0.05 if dtype == BF else 0.01) and abs(loss.item() - float(z["loss"])) < (0.02 if dtype == BF else 0.004)
        assert t_worst[0] < TEXT_REL[dtype] and t_mean < TEXT_REL_MEAN[dtype]
        assert worst[0] < ALL_REL[fixture][dtype] and mean < ALL_REL_MEAN[fixture][dtype]
        assert set(full) == {"temp", "vision_proj.bias", "visual_encoder.cls_token"} and all(x < ALL_REL[fixture][dtype] for x in full.values())


# ------------------------------------------------------------------------------------------------------------------ 2. input gradients
def _inputs(b, bt, n, width, seed=33):
    gen = torch.Generator().manual_seed(seed)
    caps = [synthetic.caption_text(900 + i, w) for i, w in enumerate((5, 11, 3)[:b])]
    ref = torch.randn((b, n, width), generator=gen)
    tgt = F.normalize(torch.randn((bt, 256), generator=gen), dim=-1)
    wl = torch.randn((b, bt), generator=gen)                                           # a loss with every logit in play
    return caps, ref, tgt, wl


def _tokens(caps):
    enc = synthetic.HashTokenizer()(list(caps))
    ids = enc.input_ids.clone()
    ids[:, 0] = 30523
    return ids, enc.attention_mask


@pytest.mark.parametrize("width", [768, 1024])
@pytest.mark.parametrize("n,b,bt", [(17, 3, 5), (577, 2, 2)])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_input_gradients_against_oracle_autograd(cuda, dtype, n, b, bt, width):
    from candidate_reranking_cir_amd.train_stage1 import stage1_train
    from tests.test_train_stage1_cpu import oracle_logits
    g, v, m1, sd1 = tiny(dtype, width)
    caps, ref, tgt, wl = _inputs(b, bt, n, width)
    ids, mask = _tokens(caps)
    m1.train()
    r, t = ref.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    logits = stage1_train(m1, r, t, ids.cuda(), mask.cuda())
    (logits * wl.cuda()).sum().backward()
    assert r.grad.shape == r.shape and t.grad.shape == t.shape and r.grad.dtype == t.grad.dtype == torch.float32
    w = {k: x.double() for k, x in sd1.items()}
    ro, to = ref.to(dtype).double().requires_grad_(True), tgt.double().requires_grad_(True)
    (oracle_logits(w, ids, mask, ro, to) * wl.double()).sum().backward()
    rel = lambda got, want: ((got.cpu().double() - want).norm() / want.norm()).item()
    e_ref, e_tgt = rel(r.grad, ro.grad), rel(t.grad, to.grad)
    every = (r.grad.abs().amax(dim=-1) > 0).all().item()                                # each of the N tokens receives a gradient
    print(f"\n[input grads {dtype} N {n} B {b} Bt {bt} Dv {width}] d ref_tokens rel {e_ref:.3e}  d target rel {e_tgt:.3e}")
    assert every and e_ref < DIN_REL["ref"][dtype] and e_tgt < DIN_REL["target"][dtype]


def test_input_gradients_repeat_under_dropout(cuda):
    from candidate_reranking_cir_amd.train_stage1 import stage1_train
    g, v, m1, _ = tiny(HF, 1024, p_drop=0.1)
    caps, ref, tgt, wl = _inputs(3, 5, 17, 1024)
    ids, mask = _tokens(caps)
    m1.train()
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        m1.zero_grad(set_to_none=True)
        r, t = ref.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
        (stage1_train(m1, r, t, ids.cuda(), mask.cuda()) * wl.cuda()).sum().backward()
        runs.append((r.grad.clone(), t.grad.clone(), m1._trainer.last_seed))
    assert runs[0][2] == runs[1][2] and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------------------------ 3. nothing else moved
def test_switch_leaves_the_text_side_alone(cuda, deterministic):
    g, v, m1, _ = tiny(HF, 768, depth=2, p_drop=0.1)
    gen = torch.Generator().manual_seed(12)
    imgs, timgs = torch.randn((3, 3, 64, 64), generator=gen).cuda(), torch.randn((3, 3, 64, 64), generator=gen).cuda()
    caps = [synthetic.caption_text(900 + i, w) for i, w in enumerate((5, 11, 3))]
    gt = torch.arange(3, device=cuda)
    m1.train()

    def step(ref, tgt):
        torch.manual_seed(9)
        m1.zero_grad(set_to_none=True)
        logits = m1.img_txt_fusion(ref, tgt, caps, train=True)
        F.cross_entropy(logits, gt).backward()
        return logits.detach().clone(), grads_of(m1)

    # graph-free inputs: the switch changes nothing
    m1.set_image_tuning(False)
    ref0, tgt0 = embed(m1, imgs, timgs)
    assert not ref0.requires_grad and not tgt0.requires_grad
    off = step(ref0, tgt0)
    m1.set_image_tuning(True)
    on = step(ref0, tgt0)
    assert len(off[1]) == 26 * 2 + 7 and off[1].keys() == on[1].keys() and torch.equal(off[0], on[0])
    assert not [n for n in off[1] if not torch.equal(off[1][n], on[1][n])]
    # a tuned step: the text side's gradients are those of a frozen step fed the same token and target values
    ref, tgt = embed(m1, imgs, timgs)
    assert ref.requires_grad and tgt.requires_grad
    tuned = step(ref, tgt)
    frozen = step(ref.detach(), tgt.detach())
    assert torch.equal(tuned[0], frozen[0]) and len(tuned[1]) == len(frozen[1]) + 2 * 12 + 6 + 2
    assert not [n for n in frozen[1] if not torch.equal(frozen[1][n], tuned[1][n])]
    # two tuned steps from the same state: the same bits in every tensor
    again = step(*embed(m1, imgs, timgs))
    assert torch.equal(tuned[0], again[0]) and tuned[1].keys() == again[1].keys()
    assert not [n for n in tuned[1] if not torch.equal(tuned[1][n], again[1][n])]


# ------------------------------------------------------------------------------------------------------------------ 4. the reference's loop
def test_reference_loop_with_both_optimizers(cuda, deterministic):
    """Three steps of stage1_train.py:144-192 (autocast, GradScaler, blip_bs = 2 mini-batches with a graph) with train.AdamW(model=...) and
    with torch.optim.AdamW.  What "the two trajectories agree within 2e-6" can mean: the first step's gradients are bit-equal in both loops
    (the GradScaler's power of two passes through every pass exactly) and the parameters after it agree to an ulp; from the second step on
    each loop runs on ITS parameters, an ulp apart, and AdamW's per-element normalisation turns the rounding noise of every element whose
    gradient is near zero (the key biases, analytically zero, first) into updates of +-lr: the loops part by up to ~lr per step whatever
    the optimizer's arithmetic (measured: 1.2e-7 after step 1; 42 tensors above 2e-6 after step 2, largest 1.7e-4, 3.2e-4 after step 3 at
    lr 1e-4, 6.5e-5 after step 3 at the lr 2e-5 used here; two train.AdamW loops repeat bit for bit; on the same gradient sequence 3.6e-7).  So the 2e-6 is asserted (a) between the two loops after the first step and
    (b) over all three steps between train.AdamW's parameters and torch.optim.AdamW stepping twin parameters through the same gradients -
    the form of the existing optimizer tests (tests/test_train_gpu.py); the three-step difference of the two loops is printed."""
    from candidate_reranking_cir_amd import train
    gen = torch.Generator().manual_seed(21)
    imgs, timgs = torch.randn((4, 3, 64, 64), generator=gen).cuda(), torch.randn((4, 3, 64, 64), generator=gen).cuda()
    caps = [synthetic.caption_text(900 + i, w) for i, w in enumerate((5, 11, 3, 8))]
    gt = torch.arange(4, device=cuda)
    kw = dict(lr=2e-5, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    ends, first, first_grads = [], [], []
    for kind in ("ours", "torch"):
        g, v, m1, sd1 = tiny(HF, 768, depth=2, p_drop=0.1)
        m1.train()
        params = [p for p in m1.parameters() if p.requires_grad]
        opt = train.AdamW(params, model=m1, **kw) if kind == "ours" else torch.optim.AdamW(params, **kw)
        scaler = torch.cuda.amp.GradScaler()
        if kind == "ours":                                                           # twins: torch.optim.AdamW on the same gradient sequence
            twins = [p.detach().clone().requires_grad_(True) for p in params]
            twin_opt = torch.optim.AdamW(twins, **kw)
        for s in range(3):                                                           # stage1_train.py:144-192, blip_bs = 2
            torch.manual_seed(40 + s)
            opt.zero_grad()
            with torch.cuda.amp.autocast():
                ref, tgt = embed(m1, imgs, timgs, 2)
                logits = m1.img_txt_fusion(ref, tgt, caps, train=True)
                loss = torch.nn.CrossEntropyLoss()(logits, gt)
            if kind == "ours":                                                       # train.AdamW scales, unscales and skips inside
                loss.backward()
                assert all(p.grad is not None for p in params)
                for q, p in zip(twins, params):
                    q.grad = p.grad.detach().clone()
                if s == 0:
                    first_grads.append([p.grad.detach().clone() for p in params])
                opt.step()
                twin_opt.step()
            else:
                scaler.scale(loss).backward()
                if s == 0:
                    scaler.unscale_(opt)
                    first_grads.append([p.grad.detach().clone() for p in params])
                scaler.step(opt)
                scaler.update()
            if s == 0:
                first.append([p.detach().clone() for p in params])
        assert torch.isfinite(loss.detach())
        if kind == "ours":
            assert opt.t == 3 and opt.skipped_steps == 0
            e_same = max((p.detach() - q.detach()).abs().max().item() for p, q in zip(params, twins))
        else:
            assert scaler.get_scale() == 65536.0                                      # no step was skipped
        same = [n for n, p in m1.named_parameters() if torch.equal(p.detach().cpu(), sd1[n].float())]
        assert not same, same                                                        # every parameter changes
        # the next img_embed in either mode runs on the stepped weights
        m1.eval()
        ev = m1.img_embed(imgs, return_pool_and_normalized=True)
        twin = tiny(HF, 768, depth=2, p_drop=0.1)[2]
        twin.load_state_dict(m1.state_dict())
        twin.eval()
        ev2 = twin.img_embed(imgs, return_pool_and_normalized=True)
        assert torch.equal(ev[0], ev2[0]) and torch.equal(ev[1], ev2[1])
        m1.train(); twin.train()
        assert torch.equal(m1.img_embed(imgs).detach(), twin.img_embed(imgs).detach())
        ends.append({n: p.detach().clone() for n, p in m1.named_parameters()})
    assert all(torch.equal(a, b) for a, b in zip(*first_grads))                       # step 1: the same bits in every gradient
    e_first = max((a - b).abs().max().item() for a, b in zip(*first))
    diff = max((ends[0][n] - ends[1][n]).abs().max().item() for n in ends[0])
    print(f"\n[loop, 3 steps] train.AdamW vs torch.optim.AdamW: same gradients, 3 steps {e_same:.3e}; two loops after step 1 {e_first:.3e}, "
          f"after step 3 {diff:.3e} (lr {kw['lr']:g})")
    assert e_same < 2e-6 and e_first < 2e-6


# ------------------------------------------------------------------------------------------------------------------ 5. guards
def test_switch_modes_and_guards(cuda):
    g, v, m1, _ = tiny(HF, 768, depth=2, tuning=False)
    assert m1.image_tuning is False
    gen = torch.Generator().manual_seed(3)
    imgs = torch.randn((3, 3, 64, 64), generator=gen).cuda()
    caps = [synthetic.caption_text(900 + i, w) for i, w in enumerate((5, 11, 3))]
    m1.train()
    tok0, pool0 = m1.img_embed(imgs, return_pool_and_normalized=True)
    assert not tok0.requires_grad and not pool0.requires_grad
    for bad in ((tok0.clone().requires_grad_(True), pool0), (tok0, pool0.clone().requires_grad_(True))):
        with pytest.raises(NotImplementedError, match="blip-img-tune"):
            m1.img_txt_fusion(*bad, caps)
    m1.eval()
    ev0 = m1.img_embed(imgs, return_pool_and_normalized=True)
    # on: survives .to() and .train() / .eval(); eval and no_grad are today's results without a graph
    assert m1.set_image_tuning() is m1 and m1.image_tuning is True
    m1 = m1.to("cuda").eval().train().eval()
    assert m1.image_tuning is True
    ev1 = m1.img_embed(imgs, return_pool_and_normalized=True)
    assert all(torch.equal(a, b) and not b.requires_grad for a, b in zip(ev0, ev1))
    m1.train()
    with torch.no_grad():
        ng = m1.img_embed(imgs, return_pool_and_normalized=True)
    assert torch.equal(ng[0], tok0) and torch.equal(ng[1], pool0) and not ng[0].requires_grad and not ng[1].requires_grad
    for bad in ((tok0.clone().requires_grad_(True), pool0), (tok0, pool0.clone().requires_grad_(True))):
        assert m1.img_txt_fusion(*bad, caps).requires_grad                            # neither refusal
    m1.zero_grad(set_to_none=True)
    # a fully frozen image side: today's results, no graph
    image_side = [p for n, p in m1.named_parameters() if n.startswith(("visual_encoder.", "vision_proj."))]
    for p in image_side:
        p.requires_grad_(False)
    fr = m1.img_embed(imgs, return_pool_and_normalized=True)
    assert torch.equal(fr[0], tok0) and torch.equal(fr[1], pool0) and not fr[0].requires_grad and not fr[1].requires_grad
    # ViT frozen, vision_proj trainable: a graph into vision_proj, none into the ViT; the features are today's bits
    m1.vision_proj.weight.requires_grad_(True)
    m1.vision_proj.bias.requires_grad_(True)
    tok, pool = m1.img_embed(imgs, return_pool_and_normalized=True)
    assert not tok.requires_grad and pool.requires_grad and torch.equal(tok, tok0) and torch.equal(pool.detach(), pool0)
    wl = torch.randn((3, 256), generator=gen).cuda()
    (pool * wl).sum().backward()
    got = sorted(n for n, p in m1.named_parameters() if p.grad is not None)
    assert got == ["vision_proj.bias", "vision_proj.weight"]
    g1 = m1.vision_proj.weight.grad.clone()
    (m1.img_embed(imgs, return_pool_and_normalized=True)[1] * wl).sum().backward()    # accumulated across calls
    assert torch.equal(m1.vision_proj.weight.grad, g1 + g1)
    # the ViT trained: a second backward through one img_embed call raises as in stage II
    for p in image_side:
        p.requires_grad_(True)
    m1.zero_grad(set_to_none=True)
    tok = m1.img_embed(imgs)
    assert tok.requires_grad
    tok.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        tok.sum().backward()


# ------------------------------------------------------------------------------------------------------------------ 6. kernels vs fp64
@pytest.mark.parametrize("b,bt,e", [(1, 1, 256), (3, 5, 256), (33, 7, 256), (5, 3, 64)])
def test_contrastive_bwd_target_against_fp64(cuda, b, bt, e):
    """dtarget[j][e] = (sum_i dlogits[i][j] p_hat[i][e]) / temp: a chain of B FMAs (each rounds once: the running sum carries at most
    B u sum|terms| to first order, u = eps32 / 2) and one division (one more rounding of the result, itself at most sum|terms| / temp).  Bound
    per element: (B + 1) u sum_i |dlogits[i][j] p_hat[i][e]| / temp, with a factor (1 + 2^-10) for the second-order terms."""
    from candidate_reranking_cir_amd import train_ops as T
    gen = torch.Generator().manual_seed(100 * b + bt)
    dl, ph, temp = torch.randn((b, bt), generator=gen), F.normalize(torch.randn((b, e), generator=gen), dim=-1), torch.tensor([0.07])
    runs = []
    for _ in range(2):
        runs.append(T.contrastive_bwd_target(dl.cuda(), ph.cuda(), temp.cuda()).cpu())
    assert torch.equal(runs[0], runs[1])
    t64 = temp.double()
    want = dl.double().t() @ ph.double() / t64
    bound = (b + 1) * U * (1 + 2.0 ** -10) * (dl.double().abs().t() @ ph.double().abs() / t64)
    err = (runs[0].double() - want).abs()
    print(f"\n[dtarget B {b} Bt {bt} E {e}] worst error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("n", [2, 17])
@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("bt", [1, 5])
def test_pooled_head_against_fp64(cuda, bt, d, n):
    """Every stage is compared with its own formula in float64 ON THE KERNEL'S fp32 INPUTS, so each bound is the round-off of that stage:
    a chain of k FMAs plus c further roundings is within (k + c) u sum|terms| (u = eps32 / 2, first order; (1 + 2^-10) covers the rest).
      t_e     = sum_k x_k W_ek + b_e                 D FMAs + 1 add:       d_t = (D + 1) u (sum_k |x_k W_ek| + |b_e|)
      inv     = 1 / max(sqrt(sum_e t_e^2), 1e-12)    relative: the sum of squares moves by 2 |t| d_t + (E + 1) u t^2 per term, the root halves
                                                     the relative error, sqrt and the division round once each:
                                                     r_inv = (sum_e (2 |t_e| d_t_e + (E + 1) u t_e^2)) / (2 sum t^2) + 2 u   (0 + 2 u when clamped)
      t_hat_e = t_e inv                              d_t_e inv + |t_hat_e| (r_inv + u)
      sd      = sum_e t_hat_e dt_hat_e               (E + 1) u sum|terms|     (E FMAs in four-wave tree order: at most E + 1 roundings a path)
      dt_e    = inv (dt_hat_e - t_hat_e sd)          inv (|t_hat_e| d_sd + 3 u (|dt_hat_e| + |t_hat_e sd|))
      dx_d    = sum_e dt_e W_ed                      E u sum|terms|
      dW_ed  += sum_i dt_ie x_id,  db_e += sum_i dt_ie     (Bt + 1) u (sum|terms| + |value before|)
    F.normalize's epsilon: one row is scaled to ||t|| = 1e-13 (bias 0), where the reference divides by the constant 1e-12 and the adjoint
    has no projection term.  The formulas themselves are checked against float64 autograd on the CPU first."""
    from candidate_reranking_cir_amd import ops, train_ops as T
    e = 256
    gen = torch.Generator().manual_seed(1000 * bt + d + n)
    tokens = torch.randn((bt, n, d), generator=gen)
    w = torch.randn((e, d), generator=gen) * 0.05
    eps_row = n == 2                                  # N = 2: zero bias and the last row scaled to ||t|| = 1e-13; N = 17: a bias, no such row
    if eps_row:
        bias = torch.zeros((e,))
        tokens[bt - 1, 0] *= 1e-13 / (tokens[bt - 1, 0] @ w.t()).norm()
    else:
        bias = torch.randn((e,), generator=gen) * 0.1
    dth = torch.randn((bt, e), generator=gen)
    dw0, db0 = torch.randn((e, d), generator=gen), torch.randn((e,), generator=gen)
    # the formulas against autograd, fp64, CPU (rows that the epsilon does not clamp, and the clamped one)
    x64 = tokens[:, 0].double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    t64 = x64 @ w64.t() + b64
    F.normalize(t64, dim=-1).backward(dth.double())
    nrm = t64.detach().norm(dim=-1)
    inv64 = 1.0 / nrm.clamp_min(1e-12)
    th64 = t64.detach() * inv64[:, None]
    sd64 = torch.where(nrm < 1e-12, torch.zeros_like(nrm), (th64 * dth.double()).sum(-1))
    dt64 = inv64[:, None] * (dth.double() - th64 * sd64[:, None])
    for got, want in ((dt64 @ w64.detach(), x64.grad), (dt64.t() @ x64.detach(), w64.grad), (dt64.sum(0), b64.grad)):
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-12 * want.abs().max().item())
    assert int((nrm < 1e-12).sum()) == int(eps_row) and (not eps_row or 0.5e-13 < nrm[bt - 1].item() < 2e-13)
    # the kernels
    tc, wc, bc = tokens.cuda(), w.cuda(), bias.cuda()
    runs = []
    for _ in range(2):
        t_hat, inv = T.pooled_head_fwd(tc[:, 0], wc, bc)
        assert torch.equal(t_hat, ops.l2_normalize(ops.linear_f32(tc[:, 0], wc, bc)))   # the bits of the two-launch forward
        dtok = torch.full((bt + 2, n, d), 7.0, device=cuda)                            # canaries: rows 1.. of every image, one image either side
        dwp, dbp = torch.full((e + 2, d), 7.0, device=cuda), torch.full((e + 8,), 7.0, device=cuda)     # canaries around dW and db
        dw, db = dwp[1:e + 1], dbp[4:e + 4]
        dw.copy_(dw0); db.copy_(db0)
        dt = T.pooled_head_bwd(dth.cuda(), t_hat, inv, tc[:, 0], wc, dw, db, dtok[1:bt + 1, 0])
        once = (dw.clone(), db.clone())
        T.pooled_head_bwd(dth.cuda(), t_hat, inv, tc[:, 0], wc, dw, db, dtok[1:bt + 1, 0])          # a second call accumulates
        assert torch.all(dtok[0] == 7.0) and torch.all(dtok[-1] == 7.0) and torch.all(dtok[1:bt + 1, 1:] == 7.0)
        assert torch.all(dwp[0] == 7.0) and torch.all(dwp[-1] == 7.0) and torch.all(dbp[:4] == 7.0) and torch.all(dbp[-4:] == 7.0)
        runs.append([x.cpu() for x in (t_hat, inv, dt, dtok[1:bt + 1, 0], once[0], once[1], dw, db)])
    for a, b2 in zip(*runs):
        assert torch.equal(a, b2)                                                      # bitwise reproducible
    t_hat, inv, dt, dx, dw1, db1, dw2, db2 = (x.double() for x in runs[0])
    k = 1 + 2.0 ** -10
    x, wd, bd, dthd = tokens[:, 0].double(), w.double(), bias.double(), dth.double()
    t = x @ wd.t() + bd
    d_t = (d + 1) * U * (x.abs() @ wd.abs().t() + bd.abs())
    n2 = (t * t).sum(-1)
    cl = n2.sqrt() < 1e-12
    r_inv = torch.where(cl, torch.zeros_like(n2), (2 * t.abs() * d_t + (e + 1) * U * t * t).sum(-1) / (2 * n2)) + 2 * U
    inv_w = 1.0 / n2.sqrt().clamp_min(1e-12)
    th_w = t * inv_w[:, None]
    b_th = k * (d_t * inv_w[:, None] + th_w.abs() * (r_inv[:, None] + U))
    assert bool(((inv - inv_w).abs() <= k * r_inv * inv_w).all()) and bool(((t_hat - th_w).abs() <= b_th).all())
    cl32 = inv >= float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1e-12, dtype=torch.float32))      # rows the fp32 forward clamped
    sd = torch.where(cl32, torch.zeros_like(inv), (t_hat * dthd).sum(-1))
    d_sd = torch.where(cl32, torch.zeros_like(inv), (e + 1) * U * (t_hat * dthd).abs().sum(-1))
    dt_w = inv[:, None] * (dthd - t_hat * sd[:, None])
    b_dt = k * inv[:, None] * (t_hat.abs() * d_sd[:, None] + 3 * U * (dthd.abs() + (t_hat * sd[:, None]).abs()))
    assert bool(((dt - dt_w).abs() <= b_dt).all())
    assert bool(((dx - dt @ wd).abs() <= k * e * U * (dt.abs() @ wd.abs())).all())
    for got, before, inc, mag in ((dw1, dw0.double(), dt.t() @ x, dt.abs().t() @ x.abs()), (db1, db0.double(), dt.sum(0), dt.abs().sum(0))):
        assert bool(((got - (before + inc)).abs() <= k * (bt + 1) * U * (mag + before.abs())).all())
    for got, before, inc, mag in ((dw2, dw1, dt.t() @ x, dt.abs().t() @ x.abs()), (db2, db1, dt.sum(0), dt.abs().sum(0))):
        assert bool(((got - (before + inc)).abs() <= k * (bt + 1) * U * (mag + before.abs())).all())
