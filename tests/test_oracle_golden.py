"""The CPU oracle (oracle/cir_oracle.py) against golden vectors produced by the real reference
(oracle/make_golden.py).  fp32 on both sides: tolerance 2e-5 absolute on O(1) activations."""
import json

import numpy as np
import pytest
import torch

from oracle import cir_oracle as O
from candidate_reranking_cir_amd import synthetic
from tests import helpers as H

ATOL = 2e-5


@pytest.fixture(scope="module")
def tiny():
    z, g, v, sd2, sd1 = H.tiny_setup()
    with torch.no_grad():
        feats = O.img_embed(sd2, H.fixture_images(z, range(14), v.image_size))
    return z, g, v, sd2, sd1, feats


def test_vit_tiny(tiny):
    z, g, v, sd2, sd1, feats = tiny
    np.testing.assert_allclose(feats[:, :3, :8].numpy(), z["index_features_slice"], atol=ATOL)
    assert abs(feats.double().sum().item() - float(z["index_features_sum"])) < 1e-2


@pytest.mark.parametrize("flavour", ["cirr", "fiq"])
def test_scoring_loop_tiny(tiny, flavour):
    z, g, v, sd2, sd1, feats = tiny
    caps = [str(c) for c in z["cirr_caps"]] if flavour == "cirr" else [H.fiq_caption(p) for p in z["fiq_caps"]]
    labels = z["labels"]
    with torch.no_grad():
        rows, grows = [], []
        for q, cap in enumerate(caps):
            ids, mask = H.tokenize([cap])
            out = O.score_queries(sd2, sd1, feats, [int(z["refs"][q])], z["cand_idx"][q:q + 1], labels[q:q + 1], ids, mask,
                                  group_index=z["groups"][q:q + 1] if flavour == "cirr" else None)
            if flavour == "cirr":
                rows.append(out[0]); grows.append(out[1])
            else:
                rows.append(out)
    logits = torch.cat(rows)
    np.testing.assert_allclose(logits.numpy(), z[f"{flavour}_logits"], atol=ATOL)
    assert (logits[0] == O.SKIP_FILL).all()          # skipped row reproduced
    if flavour == "cirr":
        glog = torch.cat(grows)
        np.testing.assert_allclose(glog.numpy(), z["cirr_group_logits"], atol=ATOL)
        r = O.recall_at(logits, labels, (1, 5, 10, 50))
        gr = O.group_recall_at(glog, z["groups"], z["targets"])
        np.testing.assert_allclose(gr + r, z["cirr_metrics"], atol=1e-4)
    else:
        np.testing.assert_allclose(O.recall_at(logits, labels, (10, 50)), z["fiq_metrics"], atol=1e-4)


def test_padded_masks(tiny):
    z, g, v, sd2, sd1, feats = tiny
    m = H.load("masks.npz")
    ids, mask = torch.tensor(m["input_ids"]), torch.tensor(m["attention_mask"])
    assert (mask == 0).any()
    with torch.no_grad():
        h1 = O.med_forward(sd1, ids, mask, feats[:3])
        h2 = O.nlvr_forward(sd2, ids, mask, h1, feats[3:6])
    np.testing.assert_allclose(h1.numpy(), m["stage1_hidden"], atol=ATOL)
    np.testing.assert_allclose(h2.numpy(), m["stage2_hidden"], atol=ATOL)


def test_metrics_large():
    m = H.load("metrics.npz")
    logits = torch.tensor(m["logits"])
    np.testing.assert_allclose(O.recall_at(logits, m["labels"], (10, 50)), m["fiq_metrics"], atol=1e-4)
    gr = O.group_recall_at(torch.tensor(m["group_logits"]), m["group_members"], m["targets"])
    r = O.recall_at(logits, m["labels"], (1, 5, 10, 50))
    np.testing.assert_allclose(gr + r, m["cirr_metrics"], atol=1e-4)


@pytest.mark.parametrize("tag", ["full224", "full224_spread"])
def test_full224(tag):
    z = H.load(tag + ".npz")
    g, v = H.geometry(H.FULL_BERT, dict(image_size=224))
    sd2, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    k = int(z["k"])
    torch.set_num_threads(8)
    with torch.no_grad():
        feats = O.img_embed(sd2, synthetic.images(range(k + 1), 224))
        np.testing.assert_allclose(feats[:, :4, :16].numpy(), z["vit_slice"], atol=1e-4)
        ids, mask = H.tokenize([synthetic.caption_text(0, 30)])
        assert ids.shape[1] == 32
        zt = O.stage1_z_t(sd1, feats[:1], ids, mask)
        np.testing.assert_allclose(zt[0, 0].numpy(), z["z_t_cls"], atol=1e-4)
        taps = []
        logits = O.img_txt_fusion_val(sd2, zt, feats[1:], ids, mask, taps=taps)
    np.testing.assert_allclose(torch.stack([t[0] for t in taps]).numpy(), z["taps0"], atol=2e-4)
    np.testing.assert_allclose(torch.stack([t[1] for t in taps]).numpy(), z["taps1"], atol=2e-4)
    np.testing.assert_allclose(logits.numpy(), z["logits"], atol=1e-4)
    assert (torch.argsort(logits, descending=True).numpy() == z["order"]).all()


def test_rank224_and_bxb224():
    """The oracle at the benchmark geometry against the reference's own loops on STRUCTURED images (rank224.npz: one
    K=50 FashionIQ-style query incl. the joined caption, one CIRR subset) and its B x B training-mode surface in eval
    mode with padding masks inside the batch (bxb224.npz, blip_stage2.py:65-99)."""
    z, b = H.load("rank224.npz"), H.load("bxb224.npz")
    g, v = H.geometry(H.FULL_BERT, dict(image_size=224))
    sd2, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    torch.set_num_threads(8)
    q = 0
    rows = [int(z["f50_refs"][q])] + [int(i) for i in z["f50_cand"][q]] + [int(i) for i in z["c100_groups"][0]] + [int(z["c100_refs"][0])]
    uniq = sorted(set(rows) | set(range(8)))
    pos = {r: i for i, r in enumerate(uniq)}
    with torch.no_grad():
        feats = O.img_embed(sd2, synthetic.scene_images(uniq, 224))
        np.testing.assert_allclose(feats[[pos[i] for i in range(8)]][:, :3, :8].numpy(), z["bank_slice"][:8], atol=1e-4)
        # FashionIQ-style K = 50
        ids, mask = H.tokenize([H.fiq_caption(z["f50_caps"][q])])
        zt = O.stage1_z_t(sd1, feats[pos[rows[0]]][None], ids, mask)
        logits = O.img_txt_fusion_val(sd2, zt, feats[[pos[i] for i in rows[1:51]]], ids, mask)
        np.testing.assert_allclose(logits.numpy(), z["f50_logits"][q], atol=2e-4)
        # CIRR subset of query 0
        ids, mask = H.tokenize([str(z["c100_caps"][0])])
        zt = O.stage1_z_t(sd1, feats[pos[rows[-1]]][None], ids, mask)
        glog = O.img_txt_fusion_val(sd2, zt, feats[[pos[i] for i in rows[51:56]]], ids, mask)
        np.testing.assert_allclose(glog.numpy(), z["c100_group_logits"][0], atol=2e-4)
        # B x B: row i = (caption i, z_t i) against the B candidates
        ids, mask = H.tokenize([str(c) for c in b["caps"]])
        assert (mask == 0).any()
        bank = feats[[pos[i] for i in range(8)]]
        zt = O.stage1_z_t(sd1, bank[:4], ids, mask)
        np.testing.assert_allclose(zt[:, 0].numpy(), b["z_t_cls"], atol=1e-4)
        out = torch.stack([O.img_txt_fusion_val(sd2, zt[i:i + 1], bank[4:8], ids[i:i + 1], mask[i:i + 1]) for i in range(4)])
    np.testing.assert_allclose(out.numpy(), b["logits"], atol=2e-4)
    # the >= 16-query regrowth of the fixture (round 5, rank224_wide.npz: same weights and bank): the CIRR subset of one K = 200 query
    zw = H.load("rank224_wide.npz")
    qw = 3
    rows_w = [int(zw["c200_refs"][qw])] + [int(i) for i in zw["c200_groups"][qw]]
    with torch.no_grad():
        fw = O.img_embed(sd2, synthetic.scene_images(rows_w, 224))
        ids, mask = H.tokenize([str(zw["c200_caps"][qw])])
        glog = O.img_txt_fusion_val(sd2, O.stage1_z_t(sd1, fw[:1], ids, mask), fw[1:], ids, mask)
    np.testing.assert_allclose(glog.numpy(), zw["c200_group_logits"][qw], atol=2e-4)
    assert int(zw["c100_labels"].any(1).sum()) == 16 and int(zw["c200_labels"].any(1).sum()) == 16 and int(zw["f50_labels"].any(1).sum()) == 16


def test_rank384_subset():
    """The oracle at the REFERENCE'S OWN geometry (384 px, 577 tokens) against rank384.npz (round 6: the reference's extract_index_features
    + generate_cirr_val_predictions): the tokens of the images involved, and the CIRR subset logits of one query (6 images: ~20 s of CPU)."""
    z = H.load("rank384.npz")
    g, v = H.geometry(H.FULL_BERT, dict(image_size=384))
    sd2, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    torch.set_num_threads(8)
    q = 1
    rows = [int(z["c100_refs"][q])] + [int(i) for i in z["c100_groups"][q]]
    with torch.no_grad():
        feats = O.img_embed(sd2, synthetic.scene_images(rows, 384))
        assert feats.shape == (6, 577, 768)
        np.testing.assert_allclose(feats[:, :3, :8].numpy(), z["bank_slice"][rows], atol=1e-4)
        ids, mask = H.tokenize([str(z["c100_caps"][q])])
        glog = O.img_txt_fusion_val(sd2, O.stage1_z_t(sd1, feats[:1], ids, mask), feats[1:], ids, mask)
    np.testing.assert_allclose(glog.numpy(), z["c100_group_logits"][q], atol=2e-4)
    assert int(z["c100_labels"].any(1).sum()) == 2 and not z["c100_labels"][2].any() and np.all(z["c100_logits"][2] == np.float32(-99999.99))
    assert z["f50_logits"].shape == (4, 50)


def test_outlier224():
    """The oracle on the OUTLIER-channel weights (tests/golden/outlier224.npz: residual stream 1e2..1e3 in three channels,
    the reference's generate_cirr_val_predictions at K = 100): image tokens incl. the outlier channels, the CIRR subset
    of query 0 and the first 12 top-K candidates of query 1."""
    z = H.load("outlier224.npz")
    g, v = H.geometry(H.FULL_BERT, dict(image_size=224))
    sd2, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    torch.set_num_threads(8)
    assert float(z["vit_stream_peak"]) > 100.0            # the fixture really carries a large-magnitude stream
    rows = [int(z["refs"][0])] + [int(i) for i in z["groups"][0]] + [int(z["refs"][1])] + [int(i) for i in z["cand"][1][:12]]
    uniq = sorted(set(rows) | set(range(8)))
    pos = {r: i for i, r in enumerate(uniq)}
    with torch.no_grad():
        feats = O.img_embed(sd2, synthetic.scene_images(uniq, 224))
        first8 = feats[[pos[i] for i in range(8)]]
        np.testing.assert_allclose(first8[:, :3, :8].numpy(), z["bank_slice"][:8], atol=2e-4)
        np.testing.assert_allclose(first8[:, :3][:, :, [17, 300, 555]].numpy(), z["bank_outlier_slice"], rtol=2e-4, atol=2e-4)
        ids, mask = H.tokenize([str(z["caps"][0])])
        zt = O.stage1_z_t(sd1, feats[pos[rows[0]]][None], ids, mask)
        glog = O.img_txt_fusion_val(sd2, zt, feats[[pos[i] for i in rows[1:6]]], ids, mask)
        np.testing.assert_allclose(glog.numpy(), z["group_logits"][0], atol=3e-4)
        ids, mask = H.tokenize([str(z["caps"][1])])
        zt = O.stage1_z_t(sd1, feats[pos[rows[6]]][None], ids, mask)
        logits = O.img_txt_fusion_val(sd2, zt, feats[[pos[i] for i in rows[7:19]]], ids, mask)
        np.testing.assert_allclose(logits.numpy(), z["logits"][1][:12], atol=3e-4)
        # outlier224_wide.npz (round 5: 16 scored queries on the same weights): the CIRR subset of one of its queries
        zw = H.load("outlier224_wide.npz")
        qw = 5
        rows_w = [int(zw["refs"][qw])] + [int(i) for i in zw["groups"][qw]]
        fw = O.img_embed(sd2, synthetic.scene_images(rows_w, 224))
        ids, mask = H.tokenize([str(zw["caps"][qw])])
        glog = O.img_txt_fusion_val(sd2, O.stage1_z_t(sd1, fw[:1], ids, mask), fw[1:], ids, mask)
        np.testing.assert_allclose(glog.numpy(), zw["group_logits"][qw], atol=3e-4)
        assert int(zw["labels"].any(1).sum()) == 16 and bool((zw["logits"][~zw["labels"].any(1)] == np.float32(-99999.99)).all())


def test_vit_large_tiny():
    """The oracle's ViT at the reference's ViT-LARGE geometry (depth 24, width 1024, 16 heads; blip.py:203-209) against the
    reference's own VisionTransformer (tests/golden/vitl_tiny.npz)."""
    from candidate_reranking_cir_amd import config, weights
    z = H.load("vitl_tiny.npz")
    v = config.VitGeometry(image_size=64, width=1024, depth=24, num_heads=16)
    sd = weights.synth_state_dict(weights._vit_spec(v), int(z["seed"]), str(z["profile"]))
    with torch.no_grad():
        y = O.vit_forward(sd, synthetic.images(z["image_ids"].tolist(), 64), n_heads=16)
    np.testing.assert_allclose(y[:, :, :16].numpy(), z["tokens_slice"], atol=1e-4)
    assert abs(y.double().sum().item() - float(z["tokens_sum"])) < 1e-1


@pytest.mark.parametrize("fixture", ["train768", "train197"])
def test_training_step_gradients(fixture):
    """(train197, round 4: the same step at B = 8 x 197 image tokens; its inputs are regenerated from the stored seed.)
    The gradient oracle (torch autograd through O.img_txt_fusion_train) against ONE training step of the
    real reference (tests/golden/train768.npz: BLIP_NLVR.train() with dropout 0, img_txt_fusion, cross-entropy, backward):
    logits, loss, the set of parameters that receive a gradient, every gradient's norm, sum and 64 sampled entries."""
    import json
    import torch.nn.functional as F
    z = H.load(fixture + ".npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    sd2, _ = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    torch.set_num_threads(8)
    if "z_t" in z.files:
        z_t_in, feats_in = torch.from_numpy(z["z_t"]), torch.from_numpy(z["feats"])
    else:
        gen = torch.Generator().manual_seed(int(z["input_seed"]))
        z_t_in = torch.randn((z["input_ids"].shape[0], z["input_ids"].shape[1], 768), generator=gen)
        feats_in = torch.randn((z["input_ids"].shape[0], int(z["n_tok"]), 768), generator=gen)
        np.testing.assert_array_equal(z_t_in[:, :2, :8].numpy(), z["z_t_slice"])
    bsz = z["input_ids"].shape[0]
    # the oracle in fp64: the fixture holds the reference's fp32 rounding alone, not the sum of two hosts' rounding.  Entries whose
    # gradient is analytically zero (cls_head.2.bias[0] sums softmax - one-hot over every row) are pure fp32 noise of either sign,
    # and that noise depends on the host CPU's vector width.
    w = {k: t.clone().double() for k, t in sd2.items()}
    keys = [k for k in w if k.startswith(("text_encoder.", "cls_head.")) and w[k].is_floating_point()]
    for k in keys:
        w[k].requires_grad_(True)
    logits = O.img_txt_fusion_train(w, z_t_in.double(), feats_in.double(), torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]))
    loss = F.cross_entropy(logits, torch.arange(bsz))
    loss.backward()
    np.testing.assert_allclose(logits.detach().numpy(), z["logits"], atol=2e-4)
    assert abs(loss.item() - float(z["loss"])) < 1e-4
    names = [str(n) for n in z["names"]]
    assert sorted(names) == sorted(k for k in keys if w[k].grad is not None)
    gmax = float(z["norms"].max())
    for i, n in enumerate(names):
        gq = w[n].grad.flatten()
        assert abs(gq.double().norm().item() - float(z["norms"][i])) < 1e-3 * float(z["norms"][i]) + 1e-7 * gmax, n
        got = gq[torch.from_numpy(H.grad_sample_index(gq.numel()))].numpy()
        np.testing.assert_allclose(got, z["samples"][i], atol=1e-3 * float(z["norms"][i]) / np.sqrt(gq.numel()) * 8 + 1e-7 * gmax, err_msg=n)
    for key in z.files:
        if key.startswith("full__"):
            np.testing.assert_allclose(w[key[6:]].grad.numpy(), z[key], atol=1e-3 * np.abs(z[key]).max() + 1e-7 * gmax, err_msg=key)


@pytest.mark.parametrize("fixture", ["train_imgtune.npz", "train_imgtune224.npz"], ids=["depth2-64px", "vitb16-224px"])
def test_training_step_gradients_with_vit_fine_tuning(fixture):
    """`--blip-img-tune` (stage2_train.py:87-92, 191-199): the oracle's autograd through O.vit_forward + O.img_txt_fusion_train against ONE
    step of the real reference with the image encoder trained (tests/golden/train_imgtune.npz, `oracle/make_golden.py train imgtune`):
    target tokens, logits, loss, the SET of parameters with a gradient (572 text-side + 30 ViT), every gradient's norm and 64 samples.
    Round 5: the same at the image encoder's REAL geometry (train_imgtune224.npz: ViT-B/16, depth 12, 224 px / 197 tokens, 150 ViT gradients)."""
    import json
    import torch.nn.functional as F
    from candidate_reranking_cir_amd import synthetic
    z = H.load(fixture)
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    sd2, _ = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    torch.set_num_threads(8)
    w = {k: t.clone().float() for k, t in sd2.items()}
    if "cls_bias_shift" in z.files:          # the fixture margin-separates cls_head's ReLU pre-activations (oracle/make_golden.py: 768-float bias shift)
        w["cls_head.0.bias"] = w["cls_head.0.bias"] - torch.from_numpy(z["cls_bias_shift"])
    keys = [k for k in w if k.startswith(("text_encoder.", "cls_head.", "visual_encoder.")) and w[k].is_floating_point()]
    for k in keys:
        w[k].requires_grad_(True)
    feats = O.vit_forward(w, synthetic.scene_images(z["image_ids"].tolist(), v.image_size))
    if "feats" in z.files:
        np.testing.assert_allclose(feats.detach().numpy(), z["feats"], atol=2e-4)
    else:
        np.testing.assert_allclose(feats.detach().numpy()[:, :6, :32], z["feats_slice"], atol=2e-4)
        assert abs(feats.detach().double().sum().item() - float(z["feats_sum"])) < 1e-5 * float(z["feats_abs_mean"]) * feats.numel()
    bsz = z["input_ids"].shape[0]
    logits = O.img_txt_fusion_train(w, torch.from_numpy(z["z_t"]), feats, torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]))
    loss = F.cross_entropy(logits, torch.arange(bsz))
    loss.backward()
    np.testing.assert_allclose(logits.detach().numpy(), z["logits"], atol=2e-4)
    assert abs(loss.item() - float(z["loss"])) < 1e-4
    names = [str(n) for n in z["names"]]
    assert sorted(names) == sorted(k for k in keys if w[k].grad is not None)
    assert sum(n.startswith("visual_encoder.") for n in names) == 6 + 12 * v.depth and sum(not n.startswith("visual_encoder.") for n in names) == 572
    gmax = float(z["norms"].max())
    for i, n in enumerate(names):
        gq = w[n].grad.flatten()
        assert abs(gq.double().norm().item() - float(z["norms"][i])) < 1e-3 * float(z["norms"][i]) + 1e-7 * gmax, n
        got = gq[torch.from_numpy(H.grad_sample_index(gq.numel()))].numpy()
        np.testing.assert_allclose(got, z["samples"][i], atol=1e-3 * float(z["norms"][i]) / np.sqrt(gq.numel()) * 8 + 1e-7 * gmax, err_msg=n)
