"""Stage-I training with a trainable image encoder, without a GPU: the two fixtures of tools/make_stage1_imgtune_golden.py load and name
the tensors the REAL reference's step gives a gradient (319 text side + the ViT's + vision_proj's two), their stored token / pooled-feature
slices are what the CPU oracle's ViT and head give from the regenerated images (so the GPU test's inputs are the reference's), the model
has the `set_image_tuning` switch, off by default, and the three new entry points are declared, bound, exported and check their arguments
before any launch."""
import json
import os

import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H

CASES = {"train_s1_imgtune": (351, 30, 4, 17, 64), "train_s1_imgtune_577": (339, 18, 2, 577, 384)}       # names, ViT names, B, N, pixels


@pytest.mark.parametrize("fixture", sorted(CASES))
def test_fixture_names_and_forward_slices(fixture):
    from oracle import cir_oracle as O
    n_names, n_vit, b, n_tok, size = CASES[fixture]
    z = H.load(fixture + ".npz")
    names = [str(n) for n in z["names"]]
    vit = [n for n in names if n.startswith("visual_encoder.")]
    assert len(names) == n_names == len(set(names)) and len(vit) == n_vit
    assert "vision_proj.weight" in names and "vision_proj.bias" in names and "temp" in names and "text_proj.weight" in names
    for n in ("visual_encoder.cls_token", "visual_encoder.pos_embed", "visual_encoder.patch_embed.proj.weight", "visual_encoder.norm.weight",
              "visual_encoder.blocks.0.attn.qkv.weight", "visual_encoder.blocks.0.mlp.fc2.bias"):
        assert n in vit, n
    assert len(names) - len(vit) - 2 == 319
    assert z["input_ids"].shape == (b, 42) and int(z["n_tok"]) == n_tok and z["logits"].shape == (b, b)
    assert z["norms"].shape == (n_names,) and z["samples"].shape == (n_names, 64) and float(z["norms"].min()) > 0.0      # no all-zero gradient
    for key, shape in (("full__temp", ()), ("full__vision_proj.bias", (256,)), ("full__visual_encoder.cls_token", (1, 1, 768))):
        assert z[key].shape == shape, key
    assert os.path.getsize(os.path.join(H.GOLDEN, fixture + ".npz")) < 200 * 1024
    # the stored forward slices: the oracle's ViT and pooled head on the regenerated images
    vit_cfg = json.loads(str(z["vit_cfg"]))
    assert vit_cfg["image_size"] == size
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), vit_cfg)
    _, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    gen = torch.Generator().manual_seed(int(z["input_seed"]))
    ri, ti = torch.randn((b, 3, size, size), generator=gen), torch.randn((b, 3, size, size), generator=gen)
    np.testing.assert_array_equal(ri[:, :, :2, :8].numpy(), z["ref_image_slice"])
    np.testing.assert_array_equal(ti[:, :, :2, :8].numpy(), z["tgt_image_slice"])
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    with torch.no_grad():
        tokens = O.vit_forward(sd1, ri)
        pooled = O.stage1_img_embed(sd1, ti)[1]
    assert tokens.shape == (b, n_tok, 768)
    assert np.abs(tokens[:, :3, :16].numpy() - z["tokens_slice"]).max() < 1e-4
    assert np.abs(pooled[:, :16].numpy() - z["pooled_slice"]).max() < 1e-5


def test_switch_exists_and_defaults_to_off():
    from candidate_reranking_cir_amd import config
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    g = config.BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256, encoder_width=128)
    v = config.VitGeometry(image_size=64, width=128, depth=1, num_heads=2)
    m = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    assert m.image_tuning is False
    assert m.set_image_tuning() is m and m.image_tuning is True
    assert m.train().eval().image_tuning is True
    assert m.set_image_tuning(False).image_tuning is False
    assert m.vit_geometry.drop_path_rate == 0.0 and v.drop_path_rate == 0.1          # blip_stage1.py:34: no DropPath; the caller's object is not edited


def test_entry_points_declared_bound_and_checked():
    from candidate_reranking_cir_amd import lib, train_ops
    from tests.test_abi import _declared
    for name in ("cir_contrastive_bwd_target", "cir_pooled_head_fwd", "cir_pooled_head_bwd"):
        assert name in _declared() and name in lib.SIGNATURES
    assert callable(train_ops.contrastive_bwd_target) and callable(train_ops.pooled_head_fwd) and callable(train_ops.pooled_head_bwd)
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    c = lib.load()
    assert c.cir_version() == 15
    EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
    P, F32 = 0x10000, 2                                 # 16-byte aligned fake device address: never dereferenced
    tgt = lambda **o: c.cir_contrastive_bwd_target(*[{**dict(dl=P, ph=P, temp=P, out=P, B=4, Bt=5, E=256, dt=F32, st=None), **o}[k]
                                                     for k in ("dl", "ph", "temp", "out", "B", "Bt", "E", "dt", "st")])
    assert tgt(dl=None) == EINVAL and tgt(out=None) == EINVAL and tgt(B=0) == EINVAL and tgt(Bt=0) == EINVAL and tgt(E=0) == EINVAL
    assert tgt(dt=0) == EDTYPE and tgt(dt=1) == EDTYPE
    assert tgt(E=2048) == ESHAPE and tgt(E=258) == ESHAPE and tgt(Bt=70000) == ESHAPE and tgt(B=50000, Bt=50000) == ESHAPE
    assert tgt(dl=P + 4) == EALIGN and tgt(out=P + 8) == EALIGN and tgt(temp=P + 2) == EALIGN
    fk = ("x", "ldx", "W", "b", "th", "inv", "Bt", "E", "D", "dt", "st")
    fwd = lambda **o: c.cir_pooled_head_fwd(*[{**dict(x=P, ldx=577 * 768, W=P, b=P, th=P, inv=P, Bt=4, E=256, D=768, dt=F32, st=None), **o}[k] for k in fk])
    assert fwd(x=None) == EINVAL and fwd(b=None) == EINVAL and fwd(inv=None) == EINVAL and fwd(Bt=0) == EINVAL and fwd(D=0) == EINVAL
    assert fwd(dt=1) == EDTYPE
    assert fwd(E=1028) == ESHAPE and fwd(D=4096) == ESHAPE and fwd(D=766) == ESHAPE and fwd(ldx=700) == ESHAPE and fwd(Bt=70000) == ESHAPE
    assert fwd(x=P + 4) == EALIGN and fwd(ldx=577 * 768 + 2) == EALIGN and fwd(W=P + 4) == EALIGN and fwd(inv=P + 2) == EALIGN
    bk = ("dth", "th", "inv", "x", "ldx", "W", "dtw", "dx", "lddx", "dW", "db", "Bt", "E", "D", "dt", "st")
    ok = dict(dth=P, th=P, inv=P, x=P, ldx=17 * 1024, W=P, dtw=P, dx=P, lddx=17 * 1024, dW=P, db=P, Bt=4, E=256, D=1024, dt=F32, st=None)
    bwd = lambda **o: c.cir_pooled_head_bwd(*[{**ok, **o}[k] for k in bk])
    assert bwd(dth=None) == EINVAL and bwd(dtw=None) == EINVAL and bwd(dW=None) == EINVAL and bwd(db=None) == EINVAL and bwd(E=0) == EINVAL
    assert bwd(dt=0) == EDTYPE
    assert bwd(lddx=1000) == ESHAPE and bwd(D=1022, ldx=1022, lddx=1022) == ESHAPE and bwd(E=6) == ESHAPE
    assert bwd(dx=P + 4) == EALIGN and bwd(lddx=17 * 1024 + 1) == EALIGN and bwd(dW=P + 8) == EALIGN and bwd(db=P + 2) == EALIGN
    assert bwd(dx=None, lddx=0, dt=1) == EDTYPE                                      # without dx (frozen ViT) the same checks apply
