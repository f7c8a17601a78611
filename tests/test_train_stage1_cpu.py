"""Stage-I training step (BLIP_Retrieval.img_txt_fusion(..., train=True) + backward) without a GPU: (a) the CPU oracle's MED forward plus
the contrastive head written out here reproduce the REAL reference's logits, loss and gradients of both fixtures (tools/
make_stage1_train_golden.py) under float64 autograd - the fixtures pin what the GPU tests compare against; (b) the head's entry points
are declared, bound and exported, and reject bad pointers, extents, alignment and dtypes before any launch."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H


def fixture_inputs(z):
    """(reference tokens, normalised target features) of a stage-I training fixture, regenerated from its seed."""
    gen = torch.Generator().manual_seed(int(z["input_seed"]))
    b = z["input_ids"].shape[0]
    ref = torch.randn((b, int(z["n_tok"]), 768), generator=gen)
    tgt = F.normalize(torch.randn((b, 256), generator=gen), dim=-1)
    np.testing.assert_array_equal(ref[:, :2, :8].numpy(), z["ref_slice"])
    np.testing.assert_array_equal(tgt[:, :8].numpy(), z["target_slice"])
    return ref, tgt


def oracle_logits(w, ids, mask, ref, tgt, drop=None):
    """blip_stage1.py:75-91 over the oracle's MED forward: F.normalize(text_proj(z_t[:, 0])) @ target^T / temp."""
    from oracle import cir_oracle as O
    h = O.med_forward(w, ids, mask, ref, drop=drop)
    p = F.normalize(h[:, 0, :] @ w["text_proj.weight"].t() + w["text_proj.bias"], dim=-1)
    return p @ tgt.t() / w["temp"]


@pytest.mark.parametrize("fixture", ["train_s1", "train_s1_577"])
def test_fixture_against_oracle_autograd_fp64(fixture):
    z = H.load(fixture + ".npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    _, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    names = [str(n) for n in z["names"]]
    assert len(names) == 319 and "temp" in names and "text_proj.weight" in names and not any(n.startswith("vision_proj") for n in names)
    assert z["input_ids"].shape[1] == 42 and int(z["attention_mask"].sum(1).max()) == 42 and int(z["attention_mask"].sum(1).min()) < 42
    w = {k: t.double() for k, t in sd1.items()}
    for n in names:
        w[n].requires_grad_(True)
    ref, tgt = fixture_inputs(z)
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    logits = oracle_logits(w, ids, mask, ref.double(), tgt.double())
    loss = F.cross_entropy(logits, torch.arange(ids.shape[0]))
    loss.backward()
    assert np.abs(logits.detach().numpy() - z["logits"]).max() < 1e-4
    assert abs(loss.item() - float(z["loss"])) < 1e-5
    gmax = float(z["norms"].max())
    for i, n in enumerate(names):
        gq = w[n].grad.flatten()
        ref_norm = float(z["norms"][i])
        if ref_norm < 1e-6 * gmax:                       # key biases: analytically zero (softmax is shift-invariant)
            assert gq.norm().item() < 1e-6 * gmax, n
            continue
        got = gq[torch.from_numpy(H.grad_sample_index(gq.numel()))].numpy()
        rms = ref_norm / np.sqrt(gq.numel())
        assert abs(gq.norm().item() - ref_norm) < 1e-4 * ref_norm, n
        assert np.sqrt(np.mean((got - z["samples"][i]) ** 2)) < 1e-4 * rms, n
    for key in z.files:
        if key.startswith("full__"):
            ref_g = z[key]
            got = w[key[6:]].grad.numpy()
            assert np.linalg.norm(got - ref_g) < 1e-4 * np.linalg.norm(ref_g), key
    assert float(z["full__temp"]) < -1.0                  # temp receives a large (negative) gradient


def test_head_entry_points_declared_bound_and_checked():
    from candidate_reranking_cir_amd import lib, train_ops
    from tests.test_abi import _declared
    for name in ("cir_contrastive_fwd", "cir_contrastive_bwd"):
        assert name in _declared() and name in lib.SIGNATURES
    assert callable(train_ops.contrastive_fwd) and callable(train_ops.contrastive_bwd)
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    c = lib.load()
    assert c.cir_version() == 15
    EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
    P = 0x10000                                         # 16-byte aligned fake device address: never dereferenced
    F32 = 2
    fwd = lambda **o: c.cir_contrastive_fwd(*[{**dict(p=P, t=P, temp=P, ph=P, inv=P, lg=P, B=4, Bt=4, E=256, dt=F32, st=None), **o}[k]
                                               for k in ("p", "t", "temp", "ph", "inv", "lg", "B", "Bt", "E", "dt", "st")])
    assert fwd(p=None) == EINVAL and fwd(temp=None) == EINVAL and fwd(lg=None) == EINVAL
    assert fwd(B=0) == EINVAL and fwd(Bt=0) == EINVAL and fwd(E=-4) == EINVAL
    assert fwd(dt=0) == EDTYPE and fwd(dt=1) == EDTYPE and fwd(dt=7) == EDTYPE
    assert fwd(E=2048) == ESHAPE and fwd(E=258) == ESHAPE and fwd(B=70000) == ESHAPE and fwd(B=50000, Bt=50000) == ESHAPE
    assert fwd(p=P + 4) == EALIGN and fwd(t=P + 8) == EALIGN and fwd(lg=P + 4) == EALIGN and fwd(temp=P + 2) == EALIGN
    keys = ("dl", "t", "temp", "ph", "inv", "dp", "scr", "dtemp", "x", "ldx", "W", "dx", "lddx", "dW", "db", "D", "B", "Bt", "E", "dt", "st")
    ok = dict(dl=P, t=P, temp=P, ph=P, inv=P, dp=P, scr=P, dtemp=P, x=P, ldx=768 * 42, W=P, dx=P, lddx=768 * 42, dW=P, db=P, D=768, B=4, Bt=5,
              E=256, dt=F32, st=None)
    bwd = lambda **o: c.cir_contrastive_bwd(*[{**ok, **o}[k] for k in keys])
    assert bwd(dl=None) == EINVAL and bwd(dtemp=None) == EINVAL and bwd(scr=None) == EINVAL and bwd(dp=None) == EINVAL
    assert bwd(W=None) == EINVAL and bwd(db=None) == EINVAL and bwd(D=0) == EINVAL and bwd(B=0) == EINVAL     # text_proj's five: all or none
    assert bwd(dt=0) == EDTYPE and bwd(dt=1) == EDTYPE
    assert bwd(E=1028) == ESHAPE and bwd(E=6) == ESHAPE and bwd(ldx=700) == ESHAPE and bwd(D=766, ldx=766, lddx=766) == ESHAPE
    assert bwd(x=P + 4) == EALIGN and bwd(ldx=768 * 42 + 2) == EALIGN and bwd(dl=P + 4) == EALIGN and bwd(dtemp=P + 1) == EALIGN
    # the head alone (no text_proj adjoint) passes the same checks
    assert bwd(x=None, W=None, dx=None, dW=None, db=None, D=0, dt=1) == EDTYPE
