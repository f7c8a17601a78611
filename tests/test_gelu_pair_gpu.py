"""cir_rows16_gelu_pair on a real MI355X: the one-pass (dz, f) = (df * gelu'(z), gelu(z)) of a checkpointed ViT block's backward against the
two kernels it replaces - `train_ops.gelu_bwd16` (cir_rows16_colsum mode 1) and `train_ops.eltwise(MODE_GELU)` (cir_eltwise mode 0) - BIT FOR
BIT, with the bias-gradient sums absent, atomic and in the fixed order, inside canary guard bands (tests/test_guard_gpu.py's `Guarded`).

Rows 1 (one row lane), 63 / 64 / 65 (the 64-row workgroup edge from both sides), 394 (197 x 2, ragged); columns 8 (one column group), 256 /
264 (the 256-column workgroup edge from both sides), 3072 / 4096 (the MLP widths of ViT-B and ViT-L).  Every row stride is padded.

z is made of the row kinds of tests/rowpass_cases.py (`rows_of`: the ViT outlier channels, zero, tiny, randn) and of rows it has no kind
for: +-large values beyond the flat tails of erf (|z| = 6, 9.5, 30, 1e4), signed zeros, and values that are subnormal in the 16-bit type.
Nothing in it is inf or NaN, so equality of the bits is meaningful everywhere.

The atomic sums are compared with the ordered ones under the reorder bound rowpass_cases.py uses for column sums: both add the same fp32
products v = df * gelu'(z) of a column to the starting value, every term passing through at most D = `depth(rows, 64)` additions, so each is
within D u (sum |v| + |start|) of the exact sum and they are within twice that of each other (+ one fp32 subnormal).  |v| is read back from
the 16-bit dz: |v| <= |dz| (1 + 2^-8) + the smallest 16-bit subnormal, which the factor 1 + 2^-7 and the additive term below cover."""
import pytest
import torch

from tests import rowpass_cases as R
from tests.test_guard_gpu import Guarded

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16
ROWS = (1, 63, 64, 65, 394)
COLS = (8, 256, 264, 3072, 4096)
PAD = 8


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    return train_ops


def _z_rows(rows, cols, dtype, seed):
    """(rows, cols) fp32 on the CPU: row r is of kind r % 8 - four kinds of rowpass_cases.rows_of scaled like pre-activations, then +-large
    rows, signed zeros and 16-bit subnormals."""
    g = torch.Generator().manual_seed(seed)
    kinds = [R.rows_of(k, rows, cols, g) for k in ("randn", "vit", "zero", "tiny")]
    big = torch.tensor([6.0, -6.0, 9.5, -9.5, 30.0, -30.0, 1e4, -1e4, 0.0, -0.0, 1e-4, -1e-4])
    large = big[torch.randint(0, len(big), (rows, cols), generator=g)]
    tiny16 = torch.finfo(dtype).smallest_normal
    sub = (torch.randint(-64, 65, (rows, cols), generator=g).float() / 128.0) * tiny16          # multiples of tiny / 128: subnormal in `dtype`
    mixed = torch.where(torch.rand((rows, cols), generator=g) < 0.5, large, 2.5 * torch.randn((rows, cols), generator=g))
    z = torch.empty((rows, cols))
    for r in range(rows):
        z[r] = (kinds[0][r] * 1.25, kinds[1][r], kinds[2][r], kinds[3][r], large[r], sub[r], mixed[r], -kinds[1][r])[r % 8]
    return z


def _padded(src, dtype):
    """`src` as a 16-bit CUDA view with row stride cols + PAD."""
    rows, cols = src.shape
    buf = torch.zeros((rows, cols + PAD), dtype=dtype, device="cuda")
    buf[:, :cols] = src.to(dtype).cuda()
    return buf[:, :cols]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_pair_equals_the_two_kernels_it_replaces(T, dtype, cols):
    assert hasattr(T, "gelu_bwd16_pair")
    for rows in ROWS:
        seed = 1000 * rows + cols
        g = torch.Generator().manual_seed(seed + 7)
        z = _padded(_z_rows(rows, cols, dtype, seed), dtype)
        df_kind = ("randn", "vit", "tiny")[(rows + cols // 8) % 3]
        df = _padded(R.rows_of(df_kind, rows, cols, g), dtype)
        assert z.stride(0) == cols + PAD and df.stride(0) == cols + PAD and bool(torch.isfinite(z.float()).all())
        # the two kernels of the unchecked backward / forward (their own outputs are contiguous)
        want_f = T.eltwise(z.contiguous(), T.MODE_GELU, out_dtype=dtype)
        want_dz = T.gelu_bwd16(df, z)
        start = torch.full((cols,), R.START, device="cuda")
        ord_ref = start.clone()
        T.gelu_bwd16(df, z, sums=ord_ref, work=T.Workspace())                            # the existing ordered form's sums
        for form in ("none", "atomic", "ordered"):
            what = f"{dtype} {rows}x{cols} sums {form}"
            gd, gf = Guarded(rows, cols, dtype, pr=3, pc=8), Guarded(rows, cols, dtype, pr=3, pc=8)
            gs = Guarded(1, cols, torch.float32, pr=2, pc=8)
            assert gd.view.stride(0) == cols + 16 and gd.view.data_ptr() % 16 == 0
            sums = None
            if form != "none":
                sums = gs.view[0]
                sums.fill_(R.START)
            work = T.Workspace() if form == "ordered" else None
            dz, f = T.gelu_bwd16_pair(df, z, sums=sums, work=work, out=gd.view, out_f=gf.view)
            torch.cuda.synchronize()
            assert dz.data_ptr() == gd.view.data_ptr() and f.data_ptr() == gf.view.data_ptr()
            assert torch.equal(dz, want_dz) and torch.equal(_bits(dz), _bits(want_dz)), what
            assert torch.equal(f, want_f) and torch.equal(_bits(f), _bits(want_f)), what
            gd.assert_intact(what + " dz")
            gf.assert_intact(what + " f")
            if form == "ordered":
                assert torch.equal(sums, ord_ref), what
            elif form == "atomic":
                absv = dz.float().abs().sum(0).double() * (1.0 + 2.0 ** -7) + rows * float(torch.finfo(dtype).smallest_normal) * 2.0 ** -7
                bound = 2.0 * R.depth(rows, 64) * R.U * (absv + R.START) + R.SUB32
                err = (sums.double() - ord_ref.double()).abs()
                worst = float((err / bound).max())
                print(f"\n[{what}] atomic vs ordered sums: worst |d| / bound {worst:.3f}")
                assert bool((err <= bound).all()), (what, worst)
            gs.assert_intact(what + " sums")
        # outputs the wrapper allocates itself: contiguous, the same bits
        dz2, f2 = T.gelu_bwd16_pair(df, z)
        assert dz2.is_contiguous() and f2.is_contiguous() and torch.equal(_bits(dz2), _bits(want_dz)) and torch.equal(_bits(f2), _bits(want_f))


def test_wrapper_refuses_what_the_family_refuses(T):
    from candidate_reranking_cir_amd.lib import CirrankError
    z = torch.zeros((4, 16), dtype=BF, device="cuda")
    with pytest.raises(AssertionError):
        T.gelu_bwd16_pair(z, z.to(HF))
    with pytest.raises(AssertionError):
        T.gelu_bwd16_pair(z, z, out_f=torch.zeros((4, 20), dtype=BF, device="cuda")[:, :16])       # row stride 20
    with pytest.raises(CirrankError):                                                               # cols % 8 (strides 16: only the extent is wrong)
        T.gelu_bwd16_pair(z[:, :12], z[:, :12], out=torch.zeros_like(z)[:, :12], out_f=torch.zeros_like(z)[:, :12])
