"""GPU: the recurrent half of the CRNN (csrc/sed_gru.hip) element by element against float64, through the C ABI -- sed_gemm_nt,
sed_gemm_tn / sed_gemm_tn_batch, sed_transpose_shift, sed_row_sums and sed_gru_pack_weights + sed_gru_seq_fwd + sed_gru_seq_bwd in
both forms the library has.  tests/test_gpu_crnn.py keeps the whole-sequence / whole-model (norm) checks.

Reference: float64 (torch, on the device) on THE OPERANDS THE KERNEL READS.  In SED_BF16 the GEMMs and the recurrence round their
fp32 operands to bf16 (round to nearest even) before the product; the reference rounds the same values the same way (torch's
.bfloat16()) and then works in float64.  No kernel of this library serves as a reference.

Gate, per element, no element left out (none of these operations has a sign decision): |got - ref| <= c * S, S = the same
contraction over absolute values (+ |bias|, |gi| where they enter); an element whose bound is 0 must be exactly right.  u = 2^-24,
SAFE = 4 over the operation counts below; nothing was set from a measurement.
  gemm_nt        a product of two bf16 values is exact in fp32 and an fp32 MFMA is a chain of fmas, so an element costs one rounding
                 per k of its chunk, one per slab of the split-K reduction, one for the bias: c = SAFE * (min(kchunk, K) + nslabs
                 + [bias]) * u with kchunk = ceil(ceil(K / ksplit) / 32) * 32 and nslabs = ceil(K / kchunk) (the header's rule).
  gemm_tn        the same with a k-step of 64: kchunk = ceil(ceil(K / ksplit) / 64) * 64.  colsum: a thread adds every eighth row
                 of its chunk, eight threads are added in a fixed order, then the slabs: c = SAFE * (ceil(kc / 8) + 8 + nslabs) * u
                 of sum_k |A[k][m]| -- on the fp32 values in both modes (the sums are taken before the bf16 rounding).
  row_sums       a lane adds every 64th column, six shuffle levels: c = SAFE * (ceil(C / 64) + 6) * u of sum |x|.
  transpose      bit for bit.
  gru forward    teacher-forced, every (b, step, direction) on its own: the kernel's own previous state hseq_got (0 at the first
                 step) is the input of one float64 step; W_hh and -- in bf16 -- the previous state as used in the product are
                 rounded as the kernel rounds them, the blend h' = n + z (h - n) uses the fp32 state.  With
                 a_g = b_hg + sum_k h_k W_g[j][k], S_g = |b_hg| + sum_k |h_k| |W_g[j][k]|:
                   e(a_g)  = (Hd + 1) u S_g                 (Hd fmas onto the bias)
                   e(x_g)  = (Hd + 2) u (|gi_g| + S_g)      (x_g = gi_g + a_g, g = r, z)
                 fast sigmoid s = rcp(1 + exp2(-x log2 e)): v_exp_f32 and v_rcp_f32 are documented at 1 ulp (<= 2u relative); the
                 argument product and the constant log2 e add |x| u each to the exponential's relative error, so
                 rel(e) <= (2 |x| + 2) u, the sum 1 + e rounds once and the reciprocal adds 2u: |ds| <= s (2 |x| + 5) u, plus
                 e(x) / 4 (sigmoid' <= 1/4).
                   e(ghn)  = e(a_n)                          (the fourth saved plane)
                   e(x_n)  = |ghn| e(r) + r e(ghn) + u (|r ghn| + |gi_n|)          (x_n = fma(r, ghn, gi_n))
                 fast tanh t = (1 - e) rcp(1 + e), e = exp2(-2 |x| log2 e): |de| <= (4 |x| + 2) u, |dt / de| <= 2, the two sums
                 and the reciprocal and the product 4u |t|: |dt| <= (8 |x| + 4 + 4 |t|) u, plus e(x_n) (tanh' <= 1).
                   e(h')   = e(n) + |h - n| e(z) + u (z |h - n| + |h'|)
                 Arguments stay below |x| ~ 8 here (gi ~ N(0, 1), |W|, |b| <= 1 / sqrt(Hd), |h| < 1), far from the range where
                 exp2 leaves the normal numbers.  Every gate is SAFE times these.
  gru backward   a pure function of dhseq, hseq, saved, pack_bwd; it is fed the forward kernel's outputs.  Per processed step
                 dh = dhseq + carry; dn = dh (1 - z)(1 - n^2); dz = dh (h_prev - n) z (1 - z); dr = dn ghn r (1 - r);
                 dgi = (dr, dz, dn), dgh = (dr, dz, dn r) -- six separate stores, six separate checks.  The carry
                 dh z + dgh . W_hh is internal: the reference rebuilds it in float64 from the kernel's own dgh_got of the step
                 before (rounded to bf16 in bf16 mode: the kernel keeps its dgh image of the step in bf16) and its own running
                 dh.  The running dh is not teacher-forced, so its bound runs along with it:
                   E' = (E + u |dh|) z + u |dh z| + (3 Hd + 1) u sum_j |dgh_j| |W_j| + u |carry|
                   e(dn) = E |(1 - z)(1 - n^2)| + u n^2 |dh (1 - z)| + 5 u |dn|      (the difference 1 - n^2 is absolute)
                   e(dz) = E |(h_prev - n) z (1 - z)| + 5 u |dz|
                   e(dr) = e(dn) |ghn r (1 - r)| + 4 u |dr|          e(dn r) = e(dn) r + u |dn r|
  untouched      outputs and workspaces start as NaN; the pad columns N .. ldc - 1, the workspace past sed_*_ws_floats and the
                 rows past B * t must still be NaN.  Operand padding that must not be read (columns K .. lda - 1 of an NT operand,
                 M .. lda - 1 / N .. ldb - 1 of a TN operand, the rows of B a shift excludes) is NaN inside the allocation: a
                 finite in-gate result proves it was not used.  Nothing here runs out of its allocation.

Forms (the case ids name them): gemm_nt / gemm_tn fp32 and bf16, split and unsplit; the recurrence: the generic fp32 and bf16
kernels for Hd = 32 .. 256 (1 .. 8 waves) in 8-row chunks, and for bf16 / Hd = 256 the two-row 16x16x32 form.  The batch sizes put
B = chunk - 1, chunk, chunk + 1 against both chunk sizes; t = 1 (no prefetch), 2, 33.

Measured max err / gate on the MI355X (summarised at the end of the module with -s; 0.25 = the operation count without its safety
factor):
  gemm_nt        fp32 0.16 (split 0.023), bf16 0.095 (split 0.009)
  gemm_tn        fp32 C 0.045 (split 0.012), bf16 C 0.014 (split 0.004); colsum 0.027 (split 0.010) in both modes
  row_sums       0.014;  transposes, batch against single calls, saved == NULL against the training call: bit for bit
  gru forward    both forms, every Hd, fp32 and bf16 alike: hseq 0.018 .. 0.019, r and z 0.07 .. 0.09, n 0.041,
                 W_hn h + b_hn 0.002 .. 0.028
  gru backward   both forms: dgi / dgh r 0.10 .. 0.12, z 0.15 .. 0.16, n 0.11 .. 0.13, n * r 0.12
No kernel missed its gate; the two-row form rounds nowhere else than the generic kernel.  The module runs in about 5 s.
"""
import ctypes
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
NAME = {F32: "f32", BF16: "bf16"}
U = 2.0 ** -24
SAFE = 4.0
NAN = float("nan")
WS_GUARD = 256                  # NaN floats behind every workspace
EXTRA_ROWS = 3                  # NaN rows behind B * t in every recurrence output
RATIOS = {}                     # (group, check) -> max err / gate


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


@pytest.fixture(scope="module", autouse=True)
def _report(L):
    L.lib().sed_config_reload()
    yield
    L.lib().sed_config_reload()         # the variables are restored by now: no form leaks into a later module
    if RATIOS:
        print("\nmax err / gate by group and check (1.0 = at the derived bound)")
        for k in sorted(RATIOS):
            print(f"  {k[0]:14s} {k[1]:30s} {RATIOS[k]:.3e}")


@pytest.fixture(autouse=True)
def _fresh_config(L):
    """autouse fixtures are set up before, and torn down after, a test's own monkeypatch: the library re-reads its environment
    before the test and again once monkeypatch has restored the variables"""
    L.lib().sed_config_reload()
    yield
    L.lib().sed_config_reload()


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def rand(g, *shape):
    return torch.rand(*shape, device="cuda", generator=g)


def opnd(dt, x):
    """the operand the MFMA sees, as float64: the fp32 value, or its bf16 rounding (round to nearest even)"""
    return x.bfloat16().double() if dt == BF16 else x.double()


def padded(g, rows, cols, ld):
    """[rows][ld] fp32, N(0, 1) in the first `cols` columns, NaN in the padding"""
    buf = torch.full((rows, ld), NAN, device="cuda")
    buf[:, :cols] = randn(g, rows, cols)
    return buf


def nan_buf(*shape):
    return torch.full(shape, NAN, device="cuda")


def all_nan(x):
    return bool(torch.isnan(x).all())


def gate(group, what, got, ref, bound, where=""):
    got, ref = got.double(), ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{what}: the reference itself is not finite"
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{group} {what} {where}: element {tuple(bad.nonzero()[0].tolist())} is NaN/inf (not written, or a canary was read)"
    err = (got - ref).abs()
    pos = bound > 0
    inexact = (~pos) & (err != 0)
    assert not bool(inexact.any()), f"{group} {what} {where}: element {tuple(inexact.nonzero()[0].tolist())} has bound 0 and is not exact"
    ratio = torch.where(pos, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    r = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[(group, what)] = max(RATIOS.get((group, what), 0.0), r)
    if r > 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{group} {what} {where}: max err/gate {r:.3e} > 1 at element {i}: got {float(got[i])!r}, ref {float(ref[i])!r}, "
                             f"gate {float(bound[i]):.3e}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    return r


# =================================================================================================================================
# 1. sed_gemm_nt
# =================================================================================================================================
def nt_split(K, ks):
    kchunk = cdiv(cdiv(K, ks), 32) * 32
    return kchunk, cdiv(K, kchunk)


def run_nt(L, dt, A, lda, Bm, ldb, bias, C, ldc, M, N, K, ks, where):
    """one sed_gemm_nt call into C (a view of a NaN buffer) and its per-element gate; A [M][lda], Bm [N][ldb] with NaN padding"""
    lib = L.lib()
    wsn = lib.sed_gemm_nt_ws_floats(M, N, ks)
    assert wsn == (ks * M * N if ks > 1 else 0)
    ws = nan_buf(wsn + WS_GUARD)
    L.check(lib.sed_gemm_nt(dt, A.data_ptr(), lda, Bm.data_ptr(), ldb, L.ptr(bias), C.data_ptr(), ldc, M, N, K, ks,
                            L.ptr(ws) if ks > 1 else None, None), "gemm_nt")
    torch.cuda.synchronize()
    assert all_nan(ws[wsn:]), f"gemm_nt {where}: write past sed_gemm_nt_ws_floats"
    a, b = opnd(dt, A[:, :K]), opnd(dt, Bm[:, :K])
    ref, S = a @ b.t(), a.abs() @ b.abs().t()
    kchunk, nslab = nt_split(K, ks)
    count = min(kchunk, K) + nslab
    if bias is not None:
        ref, S, count = ref + bias.double(), S + bias.double().abs(), count + 1
    got = torch.as_strided(C, (M, N), (ldc, 1))
    gate("gemm_nt " + NAME[dt], "C split" if nslab > 1 else "C", got, ref, SAFE * count * U * S, where)


NT_MN = [1, 31, 127, 128, 129, 257]


@pytest.mark.parametrize("K", [1, 3, 4, 31, 32, 33, 63, 65, 1000])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_nt_shapes(L, dt, K):
    """M, N in {1, 31, 127, 128, 129, 257} crossed, at one K: the 128-tile edges, the k-step of 32, the scalar tail of the vector
    loads; lda = K rounded up to 4 plus 4 (always padded), ldb = K rounded up to 4; NaN padding; bias on every other shape"""
    g = gen(100 + K)
    lda, ldb = cdiv(K, 4) * 4 + 4, cdiv(K, 4) * 4
    for i, M in enumerate(NT_MN):
        A = padded(g, M, K, lda)
        for j, N in enumerate(NT_MN):
            Bm = padded(g, N, K, ldb)
            bias = randn(g, N) if (i + j) % 2 == 0 else None
            ldc = N + 3
            C = nan_buf(M, ldc)
            run_nt(L, dt, A, lda, Bm, ldb, bias, C, ldc, M, N, K, 1, f"M{M} N{N} K{K}")
            assert all_nan(C[:, N:]), f"gemm_nt M{M} N{N} K{K}: pad columns of C written"


@pytest.mark.parametrize("K,ks,what", [(1000, 8, "divides"), (1000, 7, "does-not-divide"), (96, 16, "exceeds-K/32"),
                                       (40, 16, "fewer-slabs-than-asked"), (65, 2, "tail-slab-of-1"), (4100, 16, "long")])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_nt_split_k(L, dt, K, ks, what):
    g = gen(200 + K + ks)
    lda = ldb = cdiv(K, 4) * 4 + 4
    for M, N in [(1, 1), (96, 40), (129, 257), (257, 31)]:
        A, Bm = padded(g, M, K, lda), padded(g, N, K, ldb)
        C = nan_buf(M, N + 5)
        run_nt(L, dt, A, lda, Bm, ldb, None, C, N + 5, M, N, K, ks, f"M{M} N{N} K{K} ksplit{ks}")
        assert all_nan(C[:, N:])


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_nt_engine_sizes(L, dt):
    """the engine's own calls at bench size: the input projection (B*t = 24000 rows, K = 128, N = 768 per direction, bias, written as
    the two halves of a [24000][1536] tensor) and dm = dgi . W_ih (N = 128, K = 1536)"""
    g = gen(7)
    R = 24000
    m, W, bias = randn(g, R, 128), randn(g, 1536, 128) / 11.3, randn(g, 1536)
    gi = nan_buf(R, 1536 + 4)
    for d in range(2):
        run_nt(L, dt, m, 128, W[768 * d:768 * (d + 1)], 128, bias[768 * d:768 * (d + 1)], gi[:, 768 * d:], 1540, R, 768, 128, 1, f"input projection d{d}")
    assert all_nan(gi[:, 1536:])
    dgi, Wt = randn(g, R, 1536), randn(g, 128, 1536) / 11.3
    dm = nan_buf(R, 128)
    run_nt(L, dt, dgi, 1536, Wt, 1536, None, dm, 128, R, 128, 1536, 1, "dm")


def test_gemm_nt_refusals(L):
    lib = L.lib()
    A, Bm, C, ws, bias = nan_buf(8, 40), nan_buf(8, 40), nan_buf(8, 8), nan_buf(4 * 64 + 8), nan_buf(8)
    args = lambda lda, ldb, bias_, ks, ws_: (F32, A.data_ptr(), lda, Bm.data_ptr(), ldb, L.ptr(bias_), C.data_ptr(), 8, 8, 8, 36, ks, L.ptr(ws_), None)
    assert lib.sed_gemm_nt(*args(36, 36, bias, 2, ws)) != 0            # bias with split-K
    assert lib.sed_gemm_nt(*args(36, 36, None, 2, None)) != 0          # split-K without a workspace
    assert lib.sed_gemm_nt(*args(37, 36, None, 1, None)) != 0          # lda not a multiple of 4
    assert lib.sed_gemm_nt(*args(36, 38, None, 1, None)) != 0          # ldb not a multiple of 4
    assert lib.sed_gemm_nt(*args(32, 36, None, 1, None)) != 0          # lda < K
    assert lib.sed_gemm_nt(F32, A.data_ptr() + 4, 36, Bm.data_ptr(), 36, None, C.data_ptr(), 8, 7, 8, 36, 1, None, None) != 0   # A not 16-byte aligned
    torch.cuda.synchronize()
    assert all_nan(C) and all_nan(ws)                                  # a refused call launches nothing


# =================================================================================================================================
# 2. sed_gemm_tn, sed_gemm_tn_batch
# =================================================================================================================================
def tn_split(K, ks):
    kchunk = cdiv(cdiv(K, ks), 64) * 64
    return kchunk, cdiv(K, kchunk)


def shifted_rows(Bm, seq, shift):
    """row k of the result = row k - shift of Bm inside sequences of `seq` rows, zero outside; the rows a shift excludes are never read"""
    K, N = Bm.shape
    out = torch.zeros_like(Bm)
    v, o = Bm.view(K // seq, seq, N), out.view(K // seq, seq, N)
    if shift == 0:
        o.copy_(v)
    elif shift == 1:
        o[:, 1:] = v[:, :-1]
    else:
        o[:, :-1] = v[:, 1:]
    return out


def tn_operands(g, K, M, N, lda, ldb, seq, shift):
    """A [K][lda], B [K][ldb] with NaN padding and NaN in the rows of B that the shift excludes"""
    A, Bm = padded(g, K, M, lda), padded(g, K, N, ldb)
    if shift != 0:
        Bm.view(K // seq, seq, ldb)[:, seq - 1 if shift == 1 else 0, :] = NAN
    return A, Bm


def tn_reference(dt, A, Bm, M, N, seq, shift, ks):
    K = A.shape[0]
    a, b = opnd(dt, A[:, :M]), shifted_rows(opnd(dt, Bm[:, :N]).contiguous(), seq, shift)
    kchunk, nslab = tn_split(K, ks)
    kc = min(kchunk, K)
    ref, S = a.t() @ b, a.abs().t() @ b.abs()
    a32 = A[:, :M].double()
    return ref, SAFE * (kc + nslab) * U * S, a32.sum(0), SAFE * (cdiv(kc, 8) + 8 + nslab) * U * a32.abs().sum(0), nslab


def run_tn(L, dt, A, lda, Bm, ldb, M, N, seq, shift, ks, where, want_cs=True):
    """one sed_gemm_tn call with fresh NaN outputs and its gates; returns (C, colsum) for the bit comparison with the batch"""
    lib = L.lib()
    K = A.shape[0]
    wsn = lib.sed_gemm_tn_ws_floats(M, N, ks)
    assert wsn == (ks * (M * N + M) if ks > 1 else 0)
    ws = nan_buf(wsn + WS_GUARD)
    ldc = N + 2
    C, cs = nan_buf(M, ldc), nan_buf(M + 8)
    L.check(lib.sed_gemm_tn(dt, A.data_ptr(), lda, Bm.data_ptr(), ldb, C.data_ptr(), ldc, cs.data_ptr() if want_cs else None, M, N, K, seq, shift,
                            ks, L.ptr(ws) if ks > 1 else None, None), "gemm_tn")
    torch.cuda.synchronize()
    assert all_nan(ws[wsn:]), f"gemm_tn {where}: write past sed_gemm_tn_ws_floats"
    assert all_nan(C[:, N:]), f"gemm_tn {where}: pad columns of C written"
    assert all_nan(cs[M:]), f"gemm_tn {where}: write past colsum[M]"
    Av, Bv = torch.as_strided(A, (K, M), (lda, 1)), torch.as_strided(Bm, (K, N), (ldb, 1))
    ref, bound, csref, csbound, nslab = tn_reference(dt, Av, Bv, M, N, seq, shift, ks)
    grp = "gemm_tn " + NAME[dt]
    gate(grp, "C split" if nslab > 1 else "C", C[:, :N], ref, bound, where)
    if want_cs:
        gate(grp, "colsum split" if nslab > 1 else "colsum", cs[:M], csref, csbound, where)
    else:
        assert all_nan(cs), f"gemm_tn {where}: colsum == NULL and something was written"
    return C, cs


TN_M, TN_N = [1, 5, 127, 128, 129, 130, 768], [1, 3, 40, 128, 129, 256]
TN_PAIRS = [(1, 1), (5, 3), (127, 40), (128, 128), (129, 129), (130, 256), (768, 128)]
# (seq, number of sequences, ksplit): K = seq * nseq
TN_SEQ = [(1, 70, 1, "seq1"), (2, 50, 1, "seq2"), (13, 10, 1, "seq13"), (13, 24, 4, "seq13-split4"), (13, 24, 3, "seq13-split-does-not-divide"),
          (32, 6, 3, "seq32-split-boundary-is-a-sequence-end"), (64, 3, 1, "seq64-sequence-ends-on-k-steps"),
          (64, 4, 2, "seq64-split-boundary-is-a-sequence-end"), (750, 2, 1, "seq750"), (750, 2, 5, "seq750-split5"),
          (13, 2, 8, "ksplit-exceeds-K/64")]


@pytest.mark.parametrize("seq,nseq,ks,what", TN_SEQ, ids=[c[3] for c in TN_SEQ])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_tn_sequences(L, dt, seq, nseq, ks, what):
    """all three shifts at every (seq, K, ksplit); for seq = 1 a shifted product is exactly 0 (S = 0: the gate demands the bits of 0)"""
    g = gen(300 + seq + 7 * nseq + ks)
    K = seq * nseq
    for shift in (-1, 0, 1):
        for M, N in TN_PAIRS:
            lda, ldb = cdiv(M, 4) * 4 + 4, cdiv(N, 4) * 4
            A, Bm = tn_operands(g, K, M, N, lda, ldb, seq, shift)
            C, _ = run_tn(L, dt, A, lda, Bm, ldb, M, N, seq, shift, ks, f"M{M} N{N} K{K} seq{seq} shift{shift:+d} ksplit{ks}")
            if seq == 1 and shift != 0:
                assert bool((C[:, :N] == 0).all())


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_tn_shapes(L, dt):
    """M in {1, 5, 127, 128, 129, 130, 768} x N in {1, 3, 40, 128, 129, 256} (neither needs to be a multiple of 4, only the leading
    dimensions), shifts and split-K alternating; N > 128: two column tiles, one colsum"""
    g = gen(31)
    seq, K = 13, 130
    for i, M in enumerate(TN_M):
        for j, N in enumerate(TN_N):
            shift, ks = (i + j) % 3 - 1, 1 + (i + 2 * j) % 3
            lda, ldb = cdiv(M, 4) * 4, cdiv(N, 4) * 4 + 4
            A, Bm = tn_operands(g, K, M, N, lda, ldb, seq, shift)
            run_tn(L, dt, A, lda, Bm, ldb, M, N, seq, shift, ks, f"M{M} N{N} K{K} seq{seq} shift{shift:+d} ksplit{ks}")


@pytest.mark.parametrize("ks", [1, 3], ids=["unsplit", "split"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_tn_colsum_null(L, dt, ks):
    g = gen(32)
    for M, N in [(5, 3), (129, 256)]:
        A, Bm = tn_operands(g, 192, M, N, cdiv(M, 4) * 4, cdiv(N, 4) * 4, 32, 1)
        run_tn(L, dt, A, cdiv(M, 4) * 4, Bm, cdiv(N, 4) * 4, M, N, 32, 1, ks, f"colsum NULL M{M} N{N} ksplit{ks}", want_cs=False)


@pytest.mark.parametrize("N,shift", [(128, 0), (256, 1)], ids=["dW_ih-N128", "dW_hh-N256-shift+1"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_tn_engine_sizes(L, dt, N, shift):
    """the bench-size weight-gradient products: M = 768, K = 24000 rows in sequences of 750, ksplit = 64"""
    g = gen(33 + N)
    A, Bm = tn_operands(g, 24000, 768, N, 768, N, 750, shift)
    run_tn(L, dt, A, 768, Bm, N, 768, N, 750, shift, 64, f"bench size N{N} shift{shift:+d}")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_tn_batch_is_bit_identical_to_single_calls(L, dt):
    """1 .. 8 problems of mixed shapes, shifts, splits and strided views in one launch: each bit-identical to its single call, which
    run_tn puts under the element-wise gate"""
    lib = L.lib()
    g = gen(34)
    seq, K = 13, 13 * 24
    Abig, Bbig = padded(g, K, 2 * 96 + 4, 2 * 96 + 8), padded(g, K, 2 * 72, 2 * 72 + 4)
    # the rows a shift excludes stay finite in the shared operand: the problems of a batch use different shifts on the same rows
    probs = []          # (A view pointer, lda, B view pointer, ldb, M, N, K, seq, shift, ksplit)
    for i, (M, N, shift, ks) in enumerate([(96, 40, 0, 1), (96, 72, 1, 4), (93, 37, 0, 4), (96, 72, -1, 3), (1, 1, 1, 1), (5, 3, -1, 2),
                                           (96, 40, 1, 8), (50, 70, 0, 1)]):
        a_off, b_off = (i % 2) * 96, (i % 2) * 72
        probs.append((Abig[:, a_off:], Abig.stride(0), Bbig[:, b_off:], Bbig.stride(0), M, N, K, seq, shift, ks))
    singles = [run_tn(L, dt, A, lda, Bm, ldb, M, N, seq_, shift, ks, f"batch problem {i}")
               for i, (A, lda, Bm, ldb, M, N, K_, seq_, shift, ks) in enumerate(probs)]
    for n in range(1, 9):
        ds = (L.GemmTnDesc * n)()
        outs, keep = [], []
        for e, (A, lda, Bm, ldb, M, N, K_, seq_, shift, ks) in zip(ds, probs):
            wsn = lib.sed_gemm_tn_ws_floats(M, N, ks)
            C, cs, ws = nan_buf(M, N + 2), nan_buf(M + 8), nan_buf(wsn + WS_GUARD)
            keep.append(ws)
            e.A, e.B, e.C, e.colsum, e.workspace = A.data_ptr(), Bm.data_ptr(), C.data_ptr(), cs.data_ptr(), ws.data_ptr() if ks > 1 else None
            e.lda, e.ldb, e.ldc, e.M, e.N, e.K, e.seq, e.shift, e.ksplit = lda, ldb, N + 2, M, N, K_, seq_, shift, ks
            outs.append((C, cs, ws, wsn))
        L.check(lib.sed_gemm_tn_batch(dt, ctypes.cast(ds, ctypes.c_void_p), n, None), "gemm_tn_batch")
        torch.cuda.synchronize()
        for i, ((C1, s1), (C2, s2, ws, wsn)) in enumerate(zip(singles, outs)):
            M, N = probs[i][4], probs[i][5]
            assert torch.equal(C1[:, :N], C2[:, :N]) and torch.equal(s1[:M], s2[:M]), f"batch of {n}: problem {i} differs from its single call"
            assert all_nan(C2[:, N:]) and all_nan(s2[M:]) and all_nan(ws[wsn:]), f"batch of {n}: problem {i} wrote outside its outputs"


def test_gemm_tn_refusals(L):
    lib = L.lib()
    A, Bm, C, ws = nan_buf(26, 8), nan_buf(26, 8), nan_buf(8, 8), nan_buf(2 * 72 + 8)
    call = lambda lda, ldb, K, seq, shift, ks, ws_: lib.sed_gemm_tn(F32, A.data_ptr(), lda, Bm.data_ptr(), ldb, C.data_ptr(), 8, None, 8, 8, K, seq,
                                                                    shift, ks, L.ptr(ws_), None)
    assert call(7, 8, 26, 13, 0, 1, None) != 0       # lda < M (and not a multiple of 4)
    assert call(8, 6, 24, 12, 0, 1, None) != 0       # ldb not a multiple of 4
    assert call(8, 8, 26, 12, 0, 1, None) != 0       # K not a multiple of seq
    assert call(8, 8, 26, 13, 2, 1, None) != 0       # shift outside {-1, 0, +1}
    assert call(8, 8, 26, 13, 0, 2, None) != 0       # split-K without a workspace
    assert lib.sed_gemm_tn(F32, A.data_ptr() + 4, 8, Bm.data_ptr(), 8, C.data_ptr(), 8, None, 4, 8, 26, 13, 0, 1, None, None) != 0   # A not 16-byte aligned
    ds = (L.GemmTnDesc * 9)()
    assert lib.sed_gemm_tn_batch(F32, ctypes.cast(ds, ctypes.c_void_p), 9, None) != 0       # more than 8 problems
    assert lib.sed_gemm_tn_batch(F32, ctypes.cast(ds, ctypes.c_void_p), 0, None) != 0
    torch.cuda.synchronize()
    assert all_nan(C) and all_nan(ws)


# =================================================================================================================================
# 3. sed_transpose_shift, sed_row_sums
# =================================================================================================================================
TR_SIZES = [1, 31, 32, 33, 100]


@pytest.mark.parametrize("R", TR_SIZES)
def test_transpose_shift_is_bit_exact(L, R):
    """R, C in {1, 31, 32, 33, 100}; seq in {1, R, a divisor of R}; the three shifts; NaN in both paddings and in the source rows a shift
    excludes; the vacated columns are exactly 0"""
    g = gen(400 + R)
    divisor = {1: 1, 31: 1, 32: 8, 33: 11, 100: 25}[R]
    for Cc in TR_SIZES:
        for seq in sorted({1, R, divisor}):
            for shift in (-1, 0, 1):
                lds, ldd = Cc + 3, R + 5
                src = padded(g, R, Cc, lds)
                if shift != 0:
                    src.view(R // seq, seq, lds)[:, seq - 1 if shift == 1 else 0, :] = NAN
                dst = nan_buf(Cc, ldd)
                L.check(L.lib().sed_transpose_shift(src.data_ptr(), lds, dst.data_ptr(), ldd, R, Cc, seq, shift, None), "transpose")
                torch.cuda.synchronize()
                ref = shifted_rows(src[:, :Cc].contiguous(), seq, shift).t()
                where = f"R{R} C{Cc} seq{seq} shift{shift:+d}"
                assert bool(torch.isfinite(dst[:, :R]).all()), f"transpose {where}: a canary was read or an element not written"
                assert torch.equal(dst[:, :R], ref), f"transpose {where}: not bit-exact"
                assert all_nan(dst[:, R:]), f"transpose {where}: pad columns written"


@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 511, 512, 513, 24000])
def test_row_sums(L, Cc):
    g = gen(500 + Cc)
    for R in (1, 3, 4, 5):
        src = padded(g, R, Cc, Cc + 3)
        out = nan_buf(R + 4)
        L.check(L.lib().sed_row_sums(src.data_ptr(), Cc + 3, out.data_ptr(), R, Cc, None), "row_sums")
        torch.cuda.synchronize()
        x = src[:, :Cc].double()
        gate("row_sums", "out", out[:R], x.sum(1), SAFE * (cdiv(Cc, 64) + 6) * U * x.abs().sum(1), f"R{R} C{Cc}")
        assert all_nan(out[R:]), f"row_sums R{R} C{Cc}: write past out[R]"


# =================================================================================================================================
# 4. the recurrence
# =================================================================================================================================
def gru_forward_checks(dt, grp, where, Hd, gi, bhh, whh, hs, sv):
    """every step on its own, from the kernel's own previous state.  gi [B][t][2][3][Hd], hs [B][t][2][Hd], sv [B][t][2][4][Hd]"""
    B, t = hs.shape[:2]
    hprev = torch.zeros_like(hs)
    hprev[:, 1:, 0] = hs[:, :-1, 0]
    hprev[:, :-1, 1] = hs[:, 1:, 1]
    hop, W = opnd(dt, hprev), opnd(dt, whh).view(2, 3, Hd, Hd)
    b = bhh.view(2, 3, Hd).double()
    a = torch.einsum("btdk,dgjk->btdgj", hop, W) + b
    Sa = torch.einsum("btdk,dgjk->btdgj", hop.abs(), W.abs()) + b.abs()
    gi = gi.double()
    e_a = (Hd + 1) * U * Sa
    x_r, x_z = gi[..., 0, :] + a[..., 0, :], gi[..., 1, :] + a[..., 1, :]
    r, z = torch.sigmoid(x_r), torch.sigmoid(x_z)
    e_r = (Hd + 2) * U * (gi[..., 0, :].abs() + Sa[..., 0, :]) / 4 + r * (2 * x_r.abs() + 5) * U
    e_z = (Hd + 2) * U * (gi[..., 1, :].abs() + Sa[..., 1, :]) / 4 + z * (2 * x_z.abs() + 5) * U
    ghn, e_ghn = a[..., 2, :], e_a[..., 2, :]
    x_n = gi[..., 2, :] + r * ghn
    n = torch.tanh(x_n)
    e_n = ghn.abs() * e_r + r * e_ghn + U * ((r * ghn).abs() + gi[..., 2, :].abs()) + (8 * x_n.abs() + 4 + 4 * n.abs()) * U
    hp = hprev.double()                                   # the blend uses the fp32 state
    h = n + z * (hp - n)
    e_h = e_n + (hp - n).abs() * e_z + U * (z * (hp - n).abs() + h.abs())
    gate(grp, "fwd hseq", hs, h, SAFE * e_h, where)
    gate(grp, "fwd saved r", sv[..., 0, :], r, SAFE * e_r, where)
    gate(grp, "fwd saved z", sv[..., 1, :], z, SAFE * e_z, where)
    gate(grp, "fwd saved n", sv[..., 2, :], n, SAFE * e_n, where)
    gate(grp, "fwd saved W_hn h + b_hn", sv[..., 3, :], ghn, SAFE * e_ghn, where)


def gru_backward_checks(dt, grp, where, Hd, dh, whh, hs, sv, dgi, dgh):
    """dh, hs [B][t][2][Hd]; sv [B][t][2][4][Hd]; dgi, dgh [B][t][2][3][Hd] (the kernel's)"""
    B, t = hs.shape[:2]
    Wb = opnd(dt, whh)                                    # [2][3Hd][Hd]
    dh, hs64, sv = dh.double(), hs.double(), sv.double()
    ref = {k: torch.zeros(B, t, 2, Hd, dtype=torch.float64, device="cuda") for k in ("dr", "dz", "dn", "dnr")}
    bnd = {k: torch.zeros_like(v) for k, v in ref.items()}
    for d in range(2):
        carry = torch.zeros(B, Hd, dtype=torch.float64, device="cuda")
        E = torch.zeros_like(carry)
        for tt in (range(t - 1, -1, -1) if d == 0 else range(t)):
            tp = tt - 1 if d == 0 else tt + 1
            hp = hs64[:, tp, d] if 0 <= tp < t else torch.zeros_like(carry)
            r, z, n, ghn = (sv[:, tt, d, i] for i in range(4))
            dhr = dh[:, tt, d] + carry
            E = E + U * dhr.abs()
            dn = dhr * (1 - z) * (1 - n * n)
            e_dn = E * ((1 - z) * (1 - n * n)).abs() + U * n * n * (dhr * (1 - z)).abs() + 5 * U * dn.abs()
            dz = dhr * (hp - n) * z * (1 - z)
            e_dz = E * ((hp - n) * z * (1 - z)).abs() + 5 * U * dz.abs()
            dr = dn * ghn * r * (1 - r)
            e_dr = e_dn * (ghn * r * (1 - r)).abs() + 4 * U * dr.abs()
            dnr = dn * r
            e_dnr = e_dn * r.abs() + U * dnr.abs()
            for k, v, e in (("dr", dr, e_dr), ("dz", dz, e_dz), ("dn", dn, e_dn), ("dnr", dnr, e_dnr)):
                ref[k][:, tt, d], bnd[k][:, tt, d] = v, e
            # the carry into the next processed step, from the kernel's own dgh of this one (its LDS image: rounded in bf16 mode)
            img = opnd(dt, dgh[:, tt, d].reshape(B, 3 * Hd))
            mm, Smm = img @ Wb[d], img.abs() @ Wb[d].abs()
            carry = dhr * z + mm
            E = E * z.abs() + U * (dhr * z).abs() + (3 * Hd + 1) * U * Smm + U * carry.abs()
    for name, got, k in (("bwd dgi r", dgi[..., 0, :], "dr"), ("bwd dgi z", dgi[..., 1, :], "dz"), ("bwd dgi n", dgi[..., 2, :], "dn"),
                         ("bwd dgh r", dgh[..., 0, :], "dr"), ("bwd dgh z", dgh[..., 1, :], "dz"), ("bwd dgh n*r", dgh[..., 2, :], "dnr")):
        gate(grp, name, got, ref[k], SAFE * bnd[k], where)


def run_gru(L, dt, grp, Hd, B, t, seed):
    lib = L.lib()
    where = f"Hd{Hd} B{B} t{t}"
    g = gen(seed)
    k = 1.0 / math.sqrt(Hd)
    whh = ((rand(g, 2, 3 * Hd, Hd) * 2 - 1) * k).contiguous()
    bhh = ((rand(g, 2, 3 * Hd) * 2 - 1) * k).contiguous()
    R = B * t
    gi = randn(g, R, 6 * Hd)
    dh = randn(g, R, 2 * Hd)
    n = lib.sed_gru_pack_elems(Hd)
    assert n == 2 * 3 * Hd * Hd
    tdt = torch.float32 if dt == F32 else torch.bfloat16
    pf, pb = torch.full((n + 64,), NAN, dtype=tdt, device="cuda"), torch.full((n + 64,), NAN, dtype=tdt, device="cuda")
    L.check(lib.sed_gru_pack_weights(dt, whh[0].data_ptr(), whh[1].data_ptr(), pf.data_ptr(), pb.data_ptr(), Hd, None), "pack")
    torch.cuda.synchronize()
    # the packs are permutations of the (rounded) recurrent matrices: same multiset of values, nothing written behind them
    for p in (pf, pb):
        assert all_nan(p[n:]), f"gru pack {where}: write past sed_gru_pack_elems"
        assert torch.equal(p[:n].float().sort().values, whh.to(tdt).float().flatten().sort().values), f"gru pack {where}: not a permutation of W_hh"
    hseq, saved = nan_buf(R + EXTRA_ROWS, 2 * Hd), nan_buf(R + EXTRA_ROWS, 8 * Hd)
    L.check(lib.sed_gru_seq_fwd(dt, gi.data_ptr(), bhh.data_ptr(), pf.data_ptr(), hseq.data_ptr(), saved.data_ptr(), B, t, Hd, None), "gru fwd")
    torch.cuda.synchronize()
    assert all_nan(hseq[R:]) and all_nan(saved[R:]), f"gru fwd {where}: rows past B * t written"
    hs, sv = hseq[:R].view(B, t, 2, Hd), saved[:R].view(B, t, 2, 4, Hd)
    gru_forward_checks(dt, grp, where, Hd, gi.view(B, t, 2, 3, Hd), bhh, whh, hs, sv)
    hseq2 = nan_buf(R + EXTRA_ROWS, 2 * Hd)              # inference: saved == NULL, the same bits
    L.check(lib.sed_gru_seq_fwd(dt, gi.data_ptr(), bhh.data_ptr(), pf.data_ptr(), hseq2.data_ptr(), None, B, t, Hd, None), "gru fwd (saved NULL)")
    torch.cuda.synchronize()
    assert torch.equal(hseq2[:R], hseq[:R]) and all_nan(hseq2[R:]), f"gru fwd {where}: saved == NULL changes hseq"
    dgi, dgh = nan_buf(R + EXTRA_ROWS, 6 * Hd), nan_buf(R + EXTRA_ROWS, 6 * Hd)
    L.check(lib.sed_gru_seq_bwd(dt, dh.data_ptr(), hseq.data_ptr(), saved.data_ptr(), pb.data_ptr(), dgi.data_ptr(), dgh.data_ptr(), B, t, Hd, None),
            "gru bwd")
    torch.cuda.synchronize()
    assert all_nan(dgi[R:]) and all_nan(dgh[R:]), f"gru bwd {where}: rows past B * t written"
    gru_backward_checks(dt, grp, where, Hd, dh.view(B, t, 2, Hd), whh, hs, sv, dgi[:R].view(B, t, 2, 3, Hd), dgh[:R].view(B, t, 2, 3, Hd))


# generic kernels, 8-row chunks (everything but bf16 / Hd = 256): every Hd meets an odd B, B = 7, 8, 9 and t = 1, 2, 33
GRU_GRID = {32: [(1, 1), (7, 33), (8, 2)], 64: [(9, 33), (2, 1), (33, 2)], 96: [(3, 33), (7, 2), (17, 1)], 128: [(8, 33), (9, 2), (1, 33)],
            160: [(7, 33), (33, 1), (2, 2)], 192: [(9, 33), (8, 1), (3, 2)], 224: [(17, 33), (7, 1), (8, 2)], 256: [(33, 33), (9, 2), (7, 1)]}


@pytest.mark.parametrize("Hd", sorted(GRU_GRID))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gru_hidden_sizes(L, dt, Hd):
    """Hd / 32 = 1 .. 8 waves per workgroup: generic kernels in 8-row chunks; bf16 / Hd = 256 takes the two-row 16x16x32 form
    (chunk 2: B = 1, 2, 3 added)"""
    two_row = dt == BF16 and Hd == 256
    grp = "gru " + NAME[dt] + (" 16x16x32 2-row" if two_row else " generic")
    for i, (B, t) in enumerate(GRU_GRID[Hd] + ([(1, 33), (2, 2), (3, 33)] if two_row else [])):
        run_gru(L, dt, grp, Hd, B, t, 600 + Hd + i)


def test_gru_refusals(L):
    lib = L.lib()
    x = nan_buf(64)
    p = x.data_ptr()
    for Hd in (0, 16, 48, 288):
        assert lib.sed_gru_pack_weights(F32, p, p, p, p, Hd, None) != 0
        assert lib.sed_gru_seq_fwd(F32, p, p, p, p, p, 1, 1, Hd, None) != 0
        assert lib.sed_gru_seq_bwd(F32, p, p, p, p, p, p, 1, 1, Hd, None) != 0
    assert lib.sed_gru_seq_fwd(F32, p, p, p, p, p, 0, 1, 32, None) != 0
    assert lib.sed_gru_seq_bwd(F32, p, p, None, p, p, p, 1, 1, 32, None) != 0          # the backward pass needs `saved`
    assert lib.sed_gru_seq_fwd(F32, p, p, p, p, p, 1 << 20, 1, 256, None) != 0         # 8 GiB of `saved`: 32-bit offsets
    torch.cuda.synchronize()
    assert all_nan(x)
