"""Kernel-level parity of the TIMED bf16 kernels against the CPU oracle (not against other HIP kernels).

Every test feeds bf16-rounded operands through the C ABI and computes the expected result with oracle/cnn_oracle.py's
convolution / BatchNorm / pooling forward and backward formulas in float64 ON THE SAME ROUNDED VALUES, rounding again only
where the kernel stores bf16.  Tolerances: 2 bf16 ulps for stored bf16 tensors, 2e-3 relative for fp32 sums -- what
tests/test_gpu_kernels_ab.py uses between two HIP kernels, here with the oracle on the other side.

  sed_conv3x3_fwd (producer/consumer kernel, csrc/sed_conv_pc.hip)      spectogram_models.py:153-156 (conv + BN statistics)
  sed_conv3x3_fwd, SED_EPI_RELUBWD                                       autograd of :155-156 (train.py:102): conv2^T, ReLU gate, BN1 sums
  sed_conv3x3_fwd_c1 (block 0, conv1 rebuilt on the matrix pipe)         :153-156 of block 0
  sed_conv3x3_wgrad_fused (DZ_BN / DZ_POOL), sed_conv3x3_wgrad_fused_c1  autograd: BN / ReLU / avg-pool backward + conv weight gradient
  sed_conv3x3_dgrad_poolstats                                            autograd: conv1^T + the pooled-tensor statistics of :158
"""
import importlib

import pytest
import torch

from oracle import cnn_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [  # B, H, W, Cin, Cout   (ragged heights, single images, every width / channel pairing of the main and default nets)
    (2, 37, 64, 32, 32),
    (1, 9, 64, 32, 32),
    (3, 50, 32, 64, 64),
    (2, 33, 32, 32, 64),
    (2, 41, 16, 128, 128),
    (2, 29, 16, 64, 128),
    (2, 45, 8, 128, 128),
    # weights-from-L2 mode of the producer/consumer kernel (>= 96 in, multiple of 128 out): three / eight chunks, two output slices,
    # an image shorter than a tile, images that end on a tile boundary
    (2, 41, 16, 96, 128),
    (1, 23, 32, 128, 256),
    (2, 19, 8, 256, 128),
    (1, 5, 16, 128, 128),
    (3, 16, 16, 128, 128),
    # the bench's grid: one workgroup per CU, several tiles each with image boundaries inside the workgroups' strips
    (160, 9, 32, 64, 64),
    (300, 20, 16, 128, 128),
    # round 5: the class-default widths through the wide weight-gradient kernel (csrc/sed_wgrad_wide.hip): 4 x 8 channel groups, one strip
    # per group pair; 2 x 4; the (64 x 128) form with several cout groups
    (2, 19, 8, 512, 512),
    (1, 23, 16, 256, 256),
    (2, 19, 8, 256, 512),
]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


def rb(t):
    """bf16 round trip in float64"""
    return t.to(torch.float32).to(BF).to(torch.float64)


def nchw(t):
    """device NHWC tensor -> CPU float64 NCHW"""
    return t.detach().to(torch.float64).cpu().permute(0, 3, 1, 2).contiguous()


def cvec(v):
    return v.detach().to(torch.float64).cpu()[None, :, None, None]


def assert_bf16_close(got_nhwc, ref_nchw, what, frac_ok=0.0):
    a = nchw(got_nhwc.float())
    b = ref_nchw
    tol = 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2e-3          # 2 bf16 ulps + accumulation noise near 0
    bad = ((a - b).abs() > tol).double().mean().item()
    assert bad <= frac_ok, f"{what}: {100 * bad:.4f}% of the elements differ from the oracle by more than 2 bf16 ulps"


def assert_sums_close(got, ref, quantum, what, rtol=2e-3):
    """fp32 sums of bf16-stored values against the float64 sums of the oracle's rounded values.  Besides the relative term the
    bound admits a few elements whose bf16 rounding went the other way (fp32 vs float64 accumulation next to a rounding
    boundary): `quantum` = what one such element moves the sum by."""
    got, ref = got.double().cpu(), ref.double().cpu()
    tol = rtol * ref.abs() + 4.0 * quantum + 1e-3
    assert ((got - ref).abs() <= tol).all(), (what, float(((got - ref).abs() - tol).max()))


def pro_act(x_nchw, sc, sh):
    """relu(scale*x+shift) rounded to bf16: the BN+ReLU prologue of the loader waves"""
    return rb(torch.relu(x_nchw * cvec(sc) + cvec(sh)))


def _pack(L, w, transposed):
    lib, P = L.lib(), L.ptr
    co, ci = w.shape[0], w.shape[1]
    out = torch.empty(9 * ci * co, device="cuda", dtype=BF)
    L.check(lib.sed_pack_conv_weight(1, P(w), P(out), co, ci, co, ci, transposed, torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_forward_kernel_vs_oracle(L, B, H, W, Cin, Cout):
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H + W)
    x = torch.randn(B, H, W, Cin, device=dev, generator=g).to(BF)
    sc, sh = torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g) * 0.3
    w = torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) * 0.05
    wpack = _pack(L, w, 0)
    w_r = rb(w.double().cpu())
    nparts = lib.sed_conv_nparts(B, H, W)
    for pro in (0, 1):
        z = torch.full((B, H, W, Cout), 7.0, device=dev, dtype=BF)
        part = torch.full((nparts, 2, Cout), 3.0, device=dev)
        L.check(lib.sed_conv3x3_fwd(1, pro, 1, P(x), P(sc) if pro else None, P(sh) if pro else None, P(wpack), P(z), None, None, None,
                                    None, None, P(part), B, H, W, Cin, Cout, st))
        torch.cuda.synchronize()
        a = pro_act(nchw(x), sc, sh) if pro else nchw(x)
        z_ref = O.conv3x3_fwd(a, w_r)                                   # spectogram_models.py:132-140 on the rounded operands
        assert_bf16_close(z, z_ref, f"forward pro={pro}")
        zr = rb(z_ref)                                                  # BatchNorm statistics of the values as stored
        sums = part.double().sum(0).cpu()
        zmax = float(zr.abs().max())
        assert_sums_close(sums[0], zr.sum(dim=(0, 2, 3)), 2.0 ** -8 * zmax, "sum z")
        assert_sums_close(sums[1], (zr * zr).sum(dim=(0, 2, 3)), 2.0 ** -7 * zmax * zmax, "sum z^2")


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_data_gradient_relu_bn_epilogue_vs_oracle(L, B, H, W, Cin, Cout):
    """conv2's data gradient: g = relu'(bn1(z1)) * conv2^T(dz2) stored in bf16, sum g and sum g*xhat1 partials."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(B * 31 + H + W)
    dz = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    zref = torch.randn(B, H, W, Cin, device=dev, generator=g).to(BF)
    sc, sh = torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g) * 0.3
    mean, invstd = torch.randn(Cin, device=dev, generator=g) * 0.1, torch.rand(Cin, device=dev, generator=g) + 0.5
    w = torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) * 0.05
    wpack_t = _pack(L, w, 1)
    nparts = lib.sed_conv_nparts(B, H, W)
    out = torch.full((B, H, W, Cin), 7.0, device=dev, dtype=BF)
    part = torch.full((nparts, 2, Cin), 3.0, device=dev)
    L.check(lib.sed_conv3x3_fwd(1, 0, 2, P(dz), None, None, P(wpack_t), P(out), P(zref), P(sc), P(sh), P(mean), P(invstd), P(part),
                                B, H, W, Cout, Cin, st))
    torch.cuda.synchronize()
    zr = nchw(zref)
    gate = (zr * cvec(sc) + cvec(sh) > 0).double()
    g_ref = O.conv3x3_dgrad(nchw(dz), rb(w.double().cpu())) * gate     # autograd of F.conv2d + relu_
    assert_bf16_close(out, g_ref, "gated data gradient")
    assert torch.equal(nchw(out.float()) == 0, rb(g_ref) == 0) or float(((nchw(out.float()) == 0) != (rb(g_ref) == 0)).double().mean()) < 1e-4
    gs = rb(g_ref)
    xhat = (zr - cvec(mean)) * cvec(invstd)
    sums = part.double().sum(0).cpu()
    gmax, xmax = float(gs.abs().max()), float(xhat.abs().max())
    assert_sums_close(sums[0], gs.sum(dim=(0, 2, 3)), 2.0 ** -8 * gmax, "sum g", rtol=5e-3)
    assert_sums_close(sums[1], (gs * xhat).sum(dim=(0, 2, 3)), 2.0 ** -8 * gmax * xmax, "sum g*xhat", rtol=5e-3)


def _c1_operands(B, H, seed):
    dev = "cuda"
    g = torch.Generator(device="cuda").manual_seed(seed)
    x1 = torch.randn(B, H, 64, device=dev, generator=g) * 3.0 + 1.0
    fmean = torch.randn(64, device=dev, generator=g)
    fstd = torch.rand(64, device=dev, generator=g) + 0.5
    w1 = torch.randn(32, 1, 3, 3, device=dev, generator=g) * 0.4
    sc1, sh1 = torch.rand(32, device=dev, generator=g) + 0.5, torch.randn(32, device=dev, generator=g) * 0.3
    return g, x1, fmean, fstd, w1, sc1, sh1


def _c1_activation(x1, fmean, fstd, w1, sc1, sh1):
    """relu(bn1(conv1(x))) as the C1-mode kernels rebuild it (csrc/conv_common.h: c1mma_init / c1mma_block): z-score in fp32,
    operands bf16(scale*w1) and bf16(x), shift as bf16 hi + lo; returns (a1 rounded to bf16, pre-activation) in NCHW float64"""
    xz = ((x1 - fmean) * (1.0 / fstd)).double().cpu()[:, None]           # fp32 arithmetic as in the loader waves
    wf = rb((w1 * sc1[:, None, None, None]).double().cpu())
    hi = rb(sh1.double().cpu())
    lo = rb(sh1.double().cpu() - hi)
    pre = O.conv3x3_fwd(rb(xz), wf) + (hi + lo)[None, :, None, None]
    return rb(torch.relu(pre)), pre


def _c1_mask_bits(mask):
    """[B][H][64][2] int16 -> bool NCHW [B][32][H][64]: half g = (c >> 2) & 1, bit (c & 3) + 4*(c >> 3)"""
    mk = mask.cpu().to(torch.int32) & 0xFFFF
    c = torch.arange(32)
    half, bit = (c >> 2) & 1, (c & 3) + 4 * (c >> 3)
    return ((mk[..., half] >> bit) & 1).permute(0, 3, 1, 2).bool()


@pytest.mark.parametrize("B,H", [(2, 37), (1, 9), (3, 41), (1, 6), (2, 64)])
def test_block0_forward_c1_vs_oracle(L, B, H):
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    W, C = 64, 32
    assert lib.sed_c1_mode_supported(1, W, C, C)
    g, x1, fmean, fstd, w1, sc1, sh1 = _c1_operands(B, H, 17 * B + H)
    w2 = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    wpack = _pack(L, w2, 0)
    nparts = lib.sed_conv_nparts(B, H, W)
    z2 = torch.full((B, H, W, C), 7.0, device=dev, dtype=BF)
    part = torch.full((nparts, 2, C), 3.0, device=dev)
    mask = torch.zeros(B, H, W, 2, device=dev, dtype=torch.int16)
    L.check(lib.sed_conv3x3_fwd_c1(1, 1, P(x1), P(fmean), P(fstd), P(w1), P(sc1), P(sh1), P(wpack), P(z2), P(part), P(mask),
                                   B, H, W, C, st))
    torch.cuda.synchronize()
    a1, pre = _c1_activation(x1, fmean, fstd, w1, sc1, sh1)
    z_ref = O.conv3x3_fwd(a1, rb(w2.double().cpu()))
    assert_bf16_close(z2, z_ref, "block-0 conv2 forward (C1 mode)")
    on = _c1_mask_bits(mask)
    flips = on != (pre > 0)
    assert not flips.any() or float(pre[flips].abs().max()) < 1e-4, "conv1 ReLU decisions"
    zr = rb(z_ref)
    sums = part.double().sum(0).cpu()
    zmax = float(zr.abs().max())
    assert_sums_close(sums[0], zr.sum(dim=(0, 2, 3)), 2.0 ** -8 * zmax, "sum z2")
    assert_sums_close(sums[1], (zr * zr).sum(dim=(0, 2, 3)), 2.0 ** -7 * zmax * zmax, "sum z2^2")


def _dz_pool(dy, z, sc, sh, ca, cb, cc, pool=2):
    """BN2 / ReLU / avg-pool backward as the weight-gradient loaders produce it: dz = [bn2(z) > 0] * ca * up(dy)/4 + cb*z + cc
    (rows dropped by the pooling floor get g = 0; pool 1: up(dy)/4 -> dy)."""
    zr = nchw(z)
    gup = O.avgpool_bwd(nchw(dy), pool, zr.shape)                       # spreads dy/4, zero for the dropped rows
    gate = (zr * cvec(sc) + cvec(sh) > 0).double()
    return rb(cvec(ca) * gup * gate + cvec(cb) * zr + cvec(cc))


def _unpack_dw(L, dwp, Cout, Cin):
    lib, P = L.lib(), L.ptr
    out = torch.empty(Cout, Cin, 3, 3, device="cuda")
    L.check(lib.sed_unpack_conv_wgrad(P(dwp), P(out), Cout, Cin, Cout, Cin, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.double().cpu()


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_fused_weight_gradient_vs_oracle(L, B, H, W, Cin, Cout):
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(B * 77 + H + W)
    x = torch.randn(B, H, W, Cin, device=dev, generator=g).to(BF)
    z = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    gr = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    dy = torch.randn(B, H // 2, W // 2, Cout, device=dev, generator=g).to(BF)
    sc_i, sh_i = torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g) * 0.3
    sc_o, sh_o = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g) * 0.3
    ca, cb, cc = (torch.randn(Cout, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    n = 9 * Cin * Cout
    for mode in ("bn", "pool"):
        ws = torch.empty(lib.sed_conv_wgrad_ws_floats(B, H, W, Cin, Cout), device=dev)
        dwp = torch.full((n,), 5.0, device=dev)
        dz_out = torch.full((B, H, W, Cout), 7.0, device=dev, dtype=BF)
        if mode == "bn":       # conv1 of a block: input = pooled output of the previous block, dz1 = BN1 backward of (g, z1)
            L.check(lib.sed_conv3x3_wgrad_fused(1, 0, P(x), None, None, 2, P(gr), P(z), None, None, P(ca), P(cb), P(cc), 1, P(dz_out),
                                                P(dwp), P(ws), B, H, W, Cin, Cout, st))
            a = nchw(x)
            dz_ref = rb(cvec(ca) * nchw(gr) + cvec(cb) * nchw(z) + cvec(cc))
        else:                  # conv2: input = relu(bn1(z1)) recomputed on load, dz2 = BN2 / ReLU / pool backward of (dy, z2)
            L.check(lib.sed_conv3x3_wgrad_fused(1, 1, P(x), P(sc_i), P(sh_i), 1, P(dy), P(z), P(sc_o), P(sh_o), P(ca), P(cb), P(cc),
                                                2, P(dz_out), P(dwp), P(ws), B, H, W, Cin, Cout, st))
            a = pro_act(nchw(x), sc_i, sh_i)
            dz_ref = _dz_pool(dy, z, sc_o, sh_o, ca, cb, cc)
        torch.cuda.synchronize()
        assert_bf16_close(dz_out, dz_ref, f"dz ({mode})", frac_ok=1e-4)      # (fma vs two roundings: a bf16 boundary case now and then)
        dw_ref = O.conv3x3_wgrad(a, dz_ref)                               # autograd's conv weight gradient on the rounded operands
        dw = _unpack_dw(L, dwp, Cout, Cin)
        err = float((dw - dw_ref).abs().max()) / float(dw_ref.abs().max())
        assert err < 2e-3, (mode, err)


WIDE_SHAPES = [  # B, H, W, Cin, Cout: both workgroup forms of csrc/sed_wgrad_wide.hip ((128 x 64) and (64 x 128) channels) at every width,
    # ragged heights (last tile of an image partial, W = 8: fewer than 8 rows, i.e. the second row of every k-step pair outside the image),
    # single tiles, more strips than tiles, strips that cross images (B large, short images)
    (2, 41, 16, 128, 128), (2, 29, 16, 64, 128), (3, 16, 16, 128, 64), (1, 5, 16, 192, 128),
    (2, 45, 8, 128, 128), (1, 7, 8, 64, 128), (2, 33, 8, 128, 64), (3, 16, 8, 128, 128),
    (2, 13, 32, 128, 128), (1, 9, 32, 64, 128), (2, 4, 32, 128, 64),
    (40, 11, 16, 128, 128), (70, 19, 8, 64, 128),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout", WIDE_SHAPES)
@pytest.mark.parametrize("mode", ["bn", "pool2", "pool1", "given", "given_pro"])
def test_wide_weight_gradient_vs_oracle(L, monkeypatch, mode, B, H, W, Cin, Cout):
    """Every (dz mode, prologue) instantiation of conv_wgrad_wide_kernel against the oracle's weight gradient (autograd of
    spectogram_models.py:153-156 under train.py:102) on bf16-rounded operands; the same call with SED_WGRAD_WIDE=0 (the narrow kernel)
    must agree with it to the fp32 summation order."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(B * 131 + H * 7 + W + Cin)
    x = torch.randn(B, H, W, Cin, device=dev, generator=g).to(BF)
    z = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    gr = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    pool = 2 if mode == "pool2" else 1
    dy = torch.randn(B, H // pool, W // pool, Cout, device=dev, generator=g).to(BF)
    sc_i, sh_i = torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g) * 0.3
    sc_o, sh_o = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g) * 0.3
    ca, cb, cc = (torch.randn(Cout, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    n = 9 * Cin * Cout

    def run():
        ws = torch.full((lib.sed_conv_wgrad_ws_floats(B, H, W, Cin, Cout) + 64,), float("nan"), device=dev)      # (+ guard: no write past the slabs)
        dwp = torch.full((n,), 5.0, device=dev)
        dz_out = torch.full((B, H, W, Cout), 7.0, device=dev, dtype=BF)
        if mode == "bn":
            L.check(lib.sed_conv3x3_wgrad_fused(1, 0, P(x), None, None, 2, P(gr), P(z), None, None, P(ca), P(cb), P(cc), 1, P(dz_out),
                                                P(dwp), P(ws), B, H, W, Cin, Cout, st))
        elif mode in ("pool2", "pool1"):
            L.check(lib.sed_conv3x3_wgrad_fused(1, 1, P(x), P(sc_i), P(sh_i), 1, P(dy), P(z), P(sc_o), P(sh_o), P(ca), P(cb), P(cc),
                                                pool, P(dz_out), P(dwp), P(ws), B, H, W, Cin, Cout, st))
        else:
            pro = 1 if mode == "given_pro" else 0
            L.check(lib.sed_conv3x3_wgrad(1, pro, P(x), P(sc_i) if pro else None, P(sh_i) if pro else None, P(gr), P(dwp), P(ws),
                                          B, H, W, Cin, Cout, st))
        torch.cuda.synchronize()
        assert torch.isnan(ws[-64:]).all(), "the kernel wrote past its workspace slabs"
        return _unpack_dw(L, dwp, Cout, Cin), dz_out

    dw, dz_out = run()
    if mode == "bn":
        a, dz_ref = nchw(x), rb(cvec(ca) * nchw(gr) + cvec(cb) * nchw(z) + cvec(cc))
    elif mode in ("pool2", "pool1"):
        a, dz_ref = pro_act(nchw(x), sc_i, sh_i), _dz_pool(dy, z, sc_o, sh_o, ca, cb, cc, pool)
    else:
        a, dz_ref = (pro_act(nchw(x), sc_i, sh_i) if mode == "given_pro" else nchw(x)), nchw(gr)
    if mode in ("bn", "pool2", "pool1"):
        assert_bf16_close(dz_out, dz_ref, f"dz ({mode})", frac_ok=1e-4)
    dw_ref = O.conv3x3_wgrad(a, dz_ref)
    err = float((dw - dw_ref).abs().max()) / float(dw_ref.abs().max())
    assert err < 2e-3, (mode, err)
    monkeypatch.setenv("SED_WGRAD_WIDE", "0")
    lib.sed_config_reload()
    try:
        dw_n, dz_n = run()
    finally:
        monkeypatch.delenv("SED_WGRAD_WIDE")
        lib.sed_config_reload()
    assert float((dw - dw_n).abs().max()) <= 1e-4 * float(dw_n.abs().max()), "wide vs narrow kernel"
    if mode in ("bn", "pool2", "pool1"):
        assert torch.equal(dz_out, dz_n), "dz_out must not depend on the kernel form"


@pytest.mark.parametrize("B,H", [(2, 37), (1, 9), (3, 41), (2, 64)])
def test_block0_fused_weight_gradient_c1_vs_oracle(L, B, H):
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    W, C = 64, 32
    g, x1, fmean, fstd, w1, sc1, sh1 = _c1_operands(B, H, 23 * B + H)
    z2 = torch.randn(B, H, W, C, device=dev, generator=g).to(BF)
    dy = torch.randn(B, H // 2, W // 2, C, device=dev, generator=g).to(BF)
    sc2, sh2 = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.3
    ca, cb, cc = (torch.randn(C, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    ws = torch.empty(lib.sed_conv_wgrad_ws_floats(B, H, W, C, C), device=dev)
    dwp = torch.full((9 * C * C,), 5.0, device=dev)
    dz_out = torch.full((B, H, W, C), 7.0, device=dev, dtype=BF)
    L.check(lib.sed_conv3x3_wgrad_fused_c1(1, P(x1), P(fmean), P(fstd), P(w1), P(sc1), P(sh1), P(dy), P(z2), P(sc2), P(sh2), P(ca), P(cb),
                                           P(cc), 2, P(dz_out), P(dwp), P(ws), B, H, W, C, st))
    torch.cuda.synchronize()
    a1, _ = _c1_activation(x1, fmean, fstd, w1, sc1, sh1)
    dz_ref = _dz_pool(dy, z2, sc2, sh2, ca, cb, cc)
    assert_bf16_close(dz_out, dz_ref, "dz2 (block 0)", frac_ok=1e-4)
    dw_ref = O.conv3x3_wgrad(a1, dz_ref)
    dw = _unpack_dw(L, dwp, C, C)
    err = float((dw - dw_ref).abs().max()) / float(dw_ref.abs().max())
    assert err < 2e-3, err


@pytest.mark.parametrize("B,H,W,Cd,C", [(2, 37, 32, 64, 32), (3, 50, 16, 128, 64), (2, 45, 8, 128, 128), (1, 9, 16, 64, 64)])
def test_data_gradient_poolstats_vs_oracle(L, B, H, W, Cd, C):
    """conv1's data gradient of block b+1 = gradient dy of block b's pooled output, plus block b's pool / ReLU / BN2 backward sums
    from pooled tensors; oracle: avgpool_bwd + ReLU gate + bn_train_bwd's sums on the full-resolution z."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(7 * B + H)
    Hz, Wz = 2 * H + 1, 2 * W
    z = torch.randn(B, Hz, Wz, C, device=dev, generator=g).to(BF)
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    gamma[1] = -gamma[1]
    beta = torch.randn(C, device=dev, generator=g) * 0.3
    mean, invstd = torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5
    scale = gamma * invstd
    shift = beta - mean * scale
    dz = torch.randn(B, H, W, Cd, device=dev, generator=g).to(BF)
    w = torch.randn(Cd, C, 3, 3, device=dev, generator=g) * 0.05
    wpack_t = _pack(L, w, 1)
    y = torch.empty(B, H, W, C, device=dev, dtype=BF)
    cnt = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8)
    L.check(lib.sed_bn_relu_pool_cnt_fwd(1, P(z), P(scale), P(shift), P(y), P(cnt), B, Hz, Wz, C, st))
    nparts = lib.sed_conv_nparts(B, H, W)
    dy = torch.full((B, H, W, C), 7.0, device=dev, dtype=BF)
    part = torch.full((nparts, 2, C), 3.0, device=dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    L.check(lib.sed_conv3x3_dgrad_poolstats(1, P(dz), P(wpack_t), P(dy), P(y), P(cnt), P(scale), P(shift), P(mean), P(invstd),
                                            P(part), nparts, P(flag), B, H, W, Cd, C, st))
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    # forward twin: ConvBlock's relu + avg_pool2d (spectogram_models.py:156-158) on the same z
    zr = nchw(z)
    act = torch.relu(zr * cvec(scale) + cvec(shift))
    assert_bf16_close(y, O.avgpool_fwd(act, 2), "pooled activation")
    dy_ref = O.conv3x3_dgrad(nchw(dz), rb(w.double().cpu()))
    assert_bf16_close(dy, dy_ref, "data gradient")
    gfull = O.avgpool_bwd(nchw(dy.float()), 2, zr.shape) * (act > 0).double()       # from the dy the kernel stored
    xhat = (zr - cvec(mean)) * cvec(invstd)
    S_ref, Q_ref = gfull.sum(dim=(0, 2, 3)), (gfull * xhat).sum(dim=(0, 2, 3))
    new = part.double().sum(0).cpu()
    mag = nchw(dy.float()).abs().sum(dim=(0, 2, 3)) * 0.25                           # sum |g| bound per channel
    assert ((new[0] - S_ref).abs() <= 1e-3 * S_ref.abs() + 1e-3).all()
    # sum g*xhat: the pooled activation is bf16 (2^-9 relative, random sign), amplified by beta/gamma; xhat = O(1)
    assert ((new[1] - Q_ref).abs() <= 2e-3 * mag * 4 + 2e-2 * Q_ref.abs()).all(), float((new[1] - Q_ref).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# fused weight + data gradient (csrc/sed_bwd_fused.hip): dz exists only in LDS
# ---------------------------------------------------------------------------------------------------------------------------
FUSED_CASES = [  # B, H, workgroups (None = default: one per CU): single tiles, strips that start inside an image, strips that cross images
    (2, 37, None), (1, 9, None), (1, 3, None), (1, 1, None), (3, 50, 2), (2, 64, 3), (2, 1500, None), (5, 7, 1),
    # H % 4 == 0 with few tiles: the fused kernel cuts ceil((H + 1) / TH) tiles per image -- more slabs than the two-kernel strips;
    # sed_conv_wgrad_ws_floats() must cover them (round-3 advisor finding: out-of-bounds slab write)
    (1, 4, None), (2, 8, None), (1, 12, None),
    # the bench's grid: 256 workgroups (one per CU), several tiles each, an image boundary inside most of them and a strip that starts
    # inside an image almost everywhere (192 images x 13 rows: 4 / 7 tiles per image, 3 / 6 tiles per workgroup)
    (192, 13, None),
]


def _reload(L):
    L.lib().sed_config_reload()


GUARD = 9 * 128 * 128          # floats behind the documented workspace size: one full slab of the largest fused layer tested here


def _guarded_ws(n):
    """workspace of exactly the documented size followed by a sentinel region the kernel must not touch"""
    buf = torch.full((n + GUARD,), -12345.0, device="cuda")
    return buf, (lambda: bool((buf[n:] == -12345.0).all().item()))


# (W, Cin, Cout) of the layers the product build's fused backward covers: block 1 of the main network (csrc/sed_bwd_fused.hip;
# /root/reference/main.py:35 widths).  The W = 16 / 8 geometries of the opt-in cin-sliced kernel run from experiments/tests/ (they call these
# same test functions with GEOM_C1_EXP / GEOM_C2_EXP after `make EXPERIMENTS=1`).
GEOM_C1 = [(32, 32, 64)]
GEOM_C2 = [(32, 64, 64, 2)]     # + the block's pooling size
GEOM_C1_EXP = [(16, 64, 128), (8, 128, 128)]
GEOM_C2_EXP = [(16, 128, 128, 2), (8, 128, 128, 1), (16, 128, 128, 1)]


@pytest.mark.parametrize("W,Cin,Cout", GEOM_C1)
@pytest.mark.parametrize("B,H,nwg", FUSED_CASES)
def test_fused_backward_conv1_vs_oracle(L, monkeypatch, B, H, nwg, W, Cin, Cout):
    """conv1 of a block (32 -> 64 at W = 32, 64 -> 128 at W = 16, 128 -> 128 at W = 8): dz1 = ca*g + cb*z1 + cc (BN1 backward),
    dW1 = x (x) dz1, dy = conv1^T(dz1) -- the gradient of the previous block's pooled output -- plus that block's pooled-tensor
    statistics.  Oracle: bn backward coefficients form, conv3x3_wgrad / conv3x3_dgrad on the bf16-rounded operands."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    if W != 32 and H > 400:
        H = H // (32 // W)           # (the same pixel count as the W = 32 case)
    if W != 32 and nwg is not None:
        nwg *= Cin // 32             # SED_BWD_FUSED_BLOCKS counts workgroups: Cin/32 of them serve one strip
    if W != 32:                      # opt-in kernel (make EXPERIMENTS=1, SED_BWD_FUSED_CS=1): measured slower than the two-kernel form
        monkeypatch.setenv("SED_BWD_FUSED_CS", "1")
        _reload(L)
        if not lib.sed_conv3x3_bwd_fused_supported(1, W, Cin, Cout, 2, 0, 4):
            pytest.fail("csrc/sed_bwd_fused_cs.hip is built with make EXPERIMENTS=1 only (experiments/tests)")
    assert lib.sed_conv3x3_bwd_fused_supported(1, W, Cin, Cout, 2, 0, 4)
    if nwg is not None:
        monkeypatch.setenv("SED_BWD_FUSED_BLOCKS", str(nwg))
    _reload(L)
    g = torch.Generator(device="cuda").manual_seed(B * 57 + H)
    x = torch.randn(B, H, W, Cin, device=dev, generator=g).abs().to(BF)          # the pooled activation of the block before (>= 0)
    cnt = torch.randint(0, 5, (B, H, W, Cin), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    z = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    gr = torch.randn(B, H, W, Cout, device=dev, generator=g).to(BF)
    ca, cb, cc = (torch.randn(Cout, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    w = torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) * 0.05
    wpack_t = _pack(L, w, 1)
    gamma = torch.rand(Cin, device=dev, generator=g) + 0.5
    beta = torch.randn(Cin, device=dev, generator=g) * 0.3
    mean, invstd = torch.randn(Cin, device=dev, generator=g) * 0.1, torch.rand(Cin, device=dev, generator=g) + 0.5
    scale = gamma * invstd
    shift = beta - mean * scale
    nparts = lib.sed_conv_nparts(B, H, W)
    ws, ws_intact = _guarded_ws(lib.sed_conv_wgrad_ws_floats(B, H, W, Cin, Cout))
    for epi in (4, 0):
        dwp = torch.full((9 * Cin * Cout,), 5.0, device=dev)
        dw = torch.full((Cout, Cin, 3, 3), 5.0, device=dev)
        dx = torch.full((B, H, W, Cin), 7.0, device=dev, dtype=BF)
        part = torch.full((nparts, 2, Cin), 3.0, device=dev)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        L.check(lib.sed_conv3x3_bwd_fused(1, 0, P(x), None, None, 2, P(gr), P(z), None, None, P(ca), P(cb), P(cc), 1, P(wpack_t), P(dx), epi,
                                          P(x) if epi else None, P(cnt) if epi else None, P(scale) if epi else None, P(shift) if epi else None,
                                          P(mean) if epi else None, P(invstd) if epi else None, P(part) if epi else None, nparts,
                                          P(flag) if epi else None, P(dwp), P(ws), B, H, W, Cin, Cout, P(dw), Cout, Cin, st))
        torch.cuda.synchronize()
        assert ws_intact(), "slab written beyond sed_conv_wgrad_ws_floats()"
        dz_ref = rb(cvec(ca) * nchw(gr) + cvec(cb) * nchw(z) + cvec(cc))
        dw_ref = O.conv3x3_wgrad(nchw(x), dz_ref)
        err = float((dw.double().cpu() - dw_ref).abs().max()) / float(dw_ref.abs().max())
        assert err < 2e-3, ("dW", epi, err)
        assert torch.equal(_unpack_dw(L, dwp, Cout, Cin), dw.double().cpu())
        dx_ref = O.conv3x3_dgrad(dz_ref, rb(w.double().cpu()))
        assert_bf16_close(dx, dx_ref, f"data gradient (epi {epi})", frac_ok=2e-4)     # (a dz element on a bf16 boundary moves 9 x 32 outputs)
        if epi:
            assert int(flag.item()) == 0
            dxs = nchw(dx.float())
            c4 = nchw(cnt.float())
            S_ref = 0.25 * (dxs * c4).sum(dim=(0, 2, 3))
            Q_ref = ((dxs * nchw(x)).sum(dim=(0, 2, 3)) - 0.25 * beta.double().cpu() * (dxs * c4).sum(dim=(0, 2, 3))) / gamma.double().cpu()
            new = part.double().sum(0).cpu()
            mag = dxs.abs().sum(dim=(0, 2, 3))
            assert ((new[0] - S_ref).abs() <= 1e-3 * S_ref.abs() + 1e-5 * mag + 1e-3).all()
            assert ((new[1] - Q_ref).abs() <= 2e-3 * Q_ref.abs() + 2e-5 * mag * 8 + 1e-3).all(), float((new[1] - Q_ref).abs().max())
    if nwg is not None:
        monkeypatch.delenv("SED_BWD_FUSED_BLOCKS")
    _reload(L)


@pytest.mark.parametrize("agate", ["1", "0"])
@pytest.mark.parametrize("W,C,Cq,pool", GEOM_C2)
@pytest.mark.parametrize("B,H,nwg", FUSED_CASES)
def test_fused_backward_conv2_vs_oracle(L, monkeypatch, B, H, nwg, W, C, Cq, pool, agate):
    """conv2 of a block (64 -> 64 at W = 32, 128 -> 128 at W = 16 / 8): dz2 = BN2 / ReLU / avg-pool backward of (dy, z2) (pool 2, or
    pool 1 as in the main network's last block), dW2 = relu(bn1(z1)) (x) dz2, g1 = relu'(bn1(z1)) * conv2^T(dz2) with the BN1
    backward sums.  agate = "1" (round 5, default): the loaders gate the staged bf16 pairs of the data gradient with the ACTIVATION tile
    in LDS (a1 != 0); "0": the round-4 epilogue re-evaluates fma(z1, scale, shift) > 0 per value (SED_BF_AGATE=0) -- same oracle."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    assert C == Cq
    assert agate == "1" or W == 32, "SED_BF_AGATE is a knob of csrc/sed_bwd_fused.hip (W = 32)"
    monkeypatch.setenv("SED_BF_AGATE", agate)
    if W != 32 and H > 400:
        H = H // (32 // W)
    if W != 32 and nwg is not None:
        nwg *= C // 32
    if W != 32:
        monkeypatch.setenv("SED_BWD_FUSED_CS", "1")
        _reload(L)
        if not lib.sed_conv3x3_bwd_fused_supported_pool(1, W, C, C, 1, 1, 2, pool):
            pytest.fail("csrc/sed_bwd_fused_cs.hip is built with make EXPERIMENTS=1 only (experiments/tests)")
    assert lib.sed_conv3x3_bwd_fused_supported_pool(1, W, C, C, 1, 1, 2, pool)
    if nwg is not None:
        monkeypatch.setenv("SED_BWD_FUSED_BLOCKS", str(nwg))
    _reload(L)
    g = torch.Generator(device="cuda").manual_seed(B * 91 + H)
    z1 = torch.randn(B, H, W, C, device=dev, generator=g).to(BF)
    z2 = torch.randn(B, H, W, C, device=dev, generator=g).to(BF)
    if pool == 2:
        dy = torch.randn(B, max(H // 2, 1), W // 2, C, device=dev, generator=g).to(BF)
        if H < 2:
            dy = dy[:, :0].contiguous()
    else:
        dy = torch.randn(B, H, W, C, device=dev, generator=g).to(BF)
    sc1, sh1 = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.3
    mean1, invstd1 = torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5
    sc2, sh2 = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.3
    ca, cb, cc = (torch.randn(C, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    wpack_t = _pack(L, w, 1)
    nparts = lib.sed_conv_nparts(B, H, W)
    ws, ws_intact = _guarded_ws(lib.sed_conv_wgrad_ws_floats(B, H, W, C, C))
    dwp = torch.full((9 * C * C,), 5.0, device=dev)
    dw = torch.full((C, C, 3, 3), 5.0, device=dev)
    g1 = torch.full((B, H, W, C), 7.0, device=dev, dtype=BF)
    part = torch.full((nparts, 2, C), 3.0, device=dev)
    dyp = P(dy) if dy.numel() else P(z2)       # (H = 1: the pooled tensor is empty; every dz row is the pooling floor's dropped row)
    L.check(lib.sed_conv3x3_bwd_fused(1, 1, P(z1), P(sc1), P(sh1), 1, dyp, P(z2), P(sc2), P(sh2), P(ca), P(cb), P(cc), pool, P(wpack_t), P(g1), 2,
                                      P(z1), None, P(sc1), P(sh1), P(mean1), P(invstd1), P(part), nparts, None, P(dwp), P(ws), B, H, W, C, C,
                                      P(dw), C, C, st))
    torch.cuda.synchronize()
    assert ws_intact(), "slab written beyond sed_conv_wgrad_ws_floats()"
    a1 = pro_act(nchw(z1), sc1, sh1)
    if dy.numel():
        dz_ref = _dz_pool(dy, z2, sc2, sh2, ca, cb, cc, pool)
    else:
        dz_ref = rb(cvec(cb) * nchw(z2) + cvec(cc))
    dw_ref = O.conv3x3_wgrad(a1, dz_ref)
    err = float((dw.double().cpu() - dw_ref).abs().max()) / float(dw_ref.abs().max())
    assert err < 2e-3, ("dW", err)
    assert torch.equal(_unpack_dw(L, dwp, C, C), dw.double().cpu())
    gate = (nchw(z1) * cvec(sc1) + cvec(sh1) > 0).double()
    g_ref = O.conv3x3_dgrad(dz_ref, rb(w.double().cpu())) * gate
    assert_bf16_close(g1, g_ref, "gated data gradient", frac_ok=2e-4)
    gs = nchw(g1.float())
    xhat = (nchw(z1) - cvec(mean1)) * cvec(invstd1)
    sums = part.double().sum(0).cpu()
    gmax, xmax = float(gs.abs().max()), float(xhat.abs().max())
    assert_sums_close(sums[0], gs.sum(dim=(0, 2, 3)), 2.0 ** -8 * gmax, "sum g")
    assert_sums_close(sums[1], (gs * xhat).sum(dim=(0, 2, 3)), 2.0 ** -8 * gmax * xmax, "sum g*xhat")
    if nwg is not None:
        monkeypatch.delenv("SED_BWD_FUSED_BLOCKS")
    _reload(L)


@pytest.mark.parametrize("B,H,nwg", [(2, 37, None), (1, 9, None), (1, 3, None), (1, 1, None), (3, 41, 2), (2, 64, 3), (2, 700, None), (5, 6, 1),
                                       (1, 4, None), (2, 8, None), (192, 13, None)])
def test_block0_fused_backward_c1_vs_oracle(L, monkeypatch, B, H, nwg):
    """sed_conv3x3_bwd_fused_c1 (csrc/sed_bwd_fused_c1.hip): conv2's weight gradient of block 0 and the [A; sum g] partials of its gated
    data gradient from ONE dz2 tile in LDS.  Oracle: BN2 / ReLU / pool backward, conv3x3_wgrad on the rebuilt activation,
    conv3x3_dgrad gated with the mask bits, contracted against the bf16 input patches.
    relu_mask = NULL: the kernel gates with the activation tile it rebuilds (a1 > 0) -- checked against the oracle gated with the
    decisions the FORWARD kernel writes for the same operands (the same MFMA: no near-tie can flip)."""
    import torch.nn.functional as F
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    W, C = 64, 32
    assert lib.sed_conv3x3_bwd_fused_c1_supported(1, W, C, 2)
    if nwg is not None:
        monkeypatch.setenv("SED_BWD_FUSED_BLOCKS", str(nwg))
    _reload(L)
    g, x1, fmean, fstd, w1, sc1, sh1 = _c1_operands(B, H, 29 * B + H)
    z2 = torch.randn(B, H, W, C, device=dev, generator=g).to(BF)
    dy = torch.randn(B, max(H // 2, 1), W // 2, C, device=dev, generator=g).to(BF)
    if H < 2:
        dy = dy[:, :0].contiguous()
    sc2, sh2 = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.3
    ca, cb, cc = (torch.randn(C, device=dev, generator=g) * s for s in (1.0, 0.1, 0.1))
    w2 = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    wpack_t = _pack(L, w2, 1)
    mask = torch.randint(0, 65536, (B, H, W, 2), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    # the forward kernel's own decisions for these operands (its conv2 output is not looked at here)
    zf = torch.empty(B, H, W, C, device=dev, dtype=BF)       # (the training form, SED_EPI_STATS: the one that writes the mask)
    fpart = torch.empty(lib.sed_conv_nparts(B, H, W), 2, C, device=dev)
    L.check(lib.sed_conv3x3_fwd_c1(1, 1, P(x1), P(fmean), P(fstd), P(w1), P(sc1), P(sh1), P(_pack(L, w2, 0)), P(zf), P(fpart), P(mask),
                                   B, H, W, C, st))
    torch.cuda.synchronize()
    a1_o, pre_o = _c1_activation(x1, fmean, fstd, w1, sc1, sh1)
    flips = _c1_mask_bits(mask) != (pre_o > 0)
    assert not flips.any() or float(pre_o[flips].abs().max()) < 1e-4, "the forward's mask is not conv1's ReLU decisions"
    nparts = lib.sed_conv_dgrad_c1_nparts()
    part = torch.full((nparts, 10, C), 9.0, device=dev)
    ws, ws_intact = _guarded_ws(lib.sed_conv_wgrad_ws_floats(B, H, W, C, C))
    dwp = torch.full((9 * C * C,), 5.0, device=dev)
    dw = torch.full((C, C, 3, 3), 5.0, device=dev)
    dyp = P(dy) if dy.numel() else P(z2)
    L.check(lib.sed_conv3x3_bwd_fused_c1(1, P(x1), P(fmean), P(fstd), P(w1), P(sc1), P(sh1), dyp, P(z2), P(sc2), P(sh2), P(ca), P(cb), P(cc), 2,
                                         P(wpack_t), None, P(part), P(dwp), P(ws), B, H, W, C, P(dw), C, C, st))
    torch.cuda.synchronize()
    assert ws_intact(), "slab written beyond sed_conv_wgrad_ws_floats()"
    a1, _ = _c1_activation(x1, fmean, fstd, w1, sc1, sh1)
    dz_ref = _dz_pool(dy, z2, sc2, sh2, ca, cb, cc) if dy.numel() else rb(cvec(cb) * nchw(z2) + cvec(cc))
    dw_ref = O.conv3x3_wgrad(a1, dz_ref)
    err = float((dw.double().cpu() - dw_ref).abs().max()) / float(dw_ref.abs().max())
    assert err < 2e-3, ("dW2", err)
    assert torch.equal(_unpack_dw(L, dwp, C, C), dw.double().cpu())
    on = _c1_mask_bits(mask).double()
    gg = rb(O.conv3x3_dgrad(dz_ref, rb(w2.double().cpu())) * on)
    xz = rb(((x1 - fmean) * (1.0 / fstd)).double().cpu())
    xp = F.pad(xz, (1, 1, 1, 1))
    ref = torch.zeros(10, C, dtype=torch.float64)
    for k in range(9):
        ti, tj = divmod(k, 3)
        ref[k] = (gg * xp[:, None, ti:ti + H, tj:tj + W]).sum(dim=(0, 2, 3))
    ref[9] = gg.sum(dim=(0, 2, 3))
    got = part.double().sum(0).cpu()
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) / scale < 2e-3, float((got - ref).abs().max()) / scale
    if nwg is not None:
        monkeypatch.delenv("SED_BWD_FUSED_BLOCKS")
    _reload(L)


@pytest.mark.parametrize("a_nparts,Cout", [(1, 32), (2, 32), (3, 20), (7, 32), (256, 32), (256, 17)])
def test_c1_backward_tail_matches_the_three_kernels(L, a_nparts, Cout):
    """sed_c1_bwd_tail (round 5) = sed_sum_partials -> sed_bn_bwd_finalize_c1 -> sed_conv3x3_c1_wgrad_combine_u with the Gram statistics
    taken from sed_bn_train_finalize_c1_g instead of a second reduction of the partial rows: same formulas and rounding points, the
    partial rows of [A; sum g] summed in a different fixed order (double accumulation either way)."""
    lib, P, dev = L.lib(), L.ptr, "cuda"
    st = torch.cuda.current_stream().cuda_stream
    Cp = 32
    g = torch.Generator(device=dev).manual_seed(100 * a_nparts + Cout)
    ng = 37
    gram = torch.randn(ng, 54, device=dev, generator=g).abs() * 50.0
    w1 = torch.randn(Cout, 1, 3, 3, device=dev, generator=g) * 0.4
    gamma, beta = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g) * 0.2
    count = 1234.0
    outs = {}
    for variant in ("plain", "g"):
        scale, shift, mean, invstd = (torch.full((Cp,), 7.0, device=dev) for _ in range(4))
        gsum = torch.zeros(54, device=dev, dtype=torch.float64)
        if variant == "plain":
            L.check(lib.sed_bn_train_finalize_c1(P(gram), ng, count, P(w1), P(gamma), P(beta), None, None, 0.1, 1e-5, P(scale), P(shift), P(mean),
                                                 P(invstd), Cout, Cp, st))
        else:
            L.check(lib.sed_bn_train_finalize_c1_g(P(gram), ng, count, P(w1), P(gamma), P(beta), None, None, 0.1, 1e-5, P(scale), P(shift), P(mean),
                                                   P(invstd), Cout, Cp, P(gsum), st))
        torch.cuda.synchronize()
        outs[variant] = (scale.clone(), shift.clone(), mean.clone(), invstd.clone(), gsum.clone())
    for a, b in zip(outs["plain"][:4], outs["g"][:4]):
        assert torch.equal(a, b)
    gsum = outs["g"][4]
    assert torch.allclose(gsum, gram.double().sum(0), rtol=1e-12, atol=0)
    mean, invstd = outs["g"][2], outs["g"][3]
    a_part = torch.randn(a_nparts, 10, Cp, device=dev, generator=g)
    a_part[:, :, Cout:] = 0
    # --- the three kernels
    a_sum = torch.empty(10, Cp, device=dev)
    L.check(lib.sed_sum_partials(P(a_part), a_nparts, 10 * Cp, P(a_sum), st))
    dgamma, dbeta = torch.full((Cp,), 3.0, device=dev), torch.full((Cp,), 3.0, device=dev)
    ca, cb, cc = (torch.full((Cp,), 5.0, device=dev) for _ in range(3))
    L.check(lib.sed_bn_bwd_finalize_c1(P(a_sum[9]), 1, count, P(a_sum), P(w1), P(gamma), P(mean), P(invstd), P(dgamma), P(dbeta), P(ca), P(cb), P(cc),
                                       Cout, Cp, st))
    dwp, dw = torch.full((9 * Cp,), 9.0, device=dev), torch.full((Cout, 1, 3, 3), 9.0, device=dev)
    L.check(lib.sed_conv3x3_c1_wgrad_combine_u(P(a_sum), P(gram), ng, P(w1), P(ca), P(cb), P(cc), P(dwp), Cout, Cp, P(dw), st))
    # --- one launch
    a_sum2 = torch.empty(10, Cp, device=dev)
    dgamma2, dbeta2 = torch.full((Cp,), 3.0, device=dev), torch.full((Cp,), 3.0, device=dev)
    ca2, cb2, cc2 = (torch.full((Cp,), 5.0, device=dev) for _ in range(3))
    dwp2, dw2 = torch.full((9 * Cp,), 9.0, device=dev), torch.full((Cout, 1, 3, 3), 9.0, device=dev)
    L.check(lib.sed_c1_bwd_tail(P(a_part), a_nparts, P(gsum), count, P(w1), P(gamma), P(mean), P(invstd), P(dgamma2), P(dbeta2), P(ca2), P(cb2), P(cc2),
                                P(a_sum2), P(dwp2), Cout, Cp, P(dw2), st))
    torch.cuda.synchronize()

    def close(x, y, what):
        sc = float(x.abs().max()) + 1e-30
        assert float((x - y).abs().max()) / sc < 2e-6, (what, float((x - y).abs().max()) / sc)

    close(a_sum, a_sum2, "a_sum")
    close(dgamma[:Cout], dgamma2[:Cout], "dgamma")
    close(dbeta[:Cout], dbeta2[:Cout], "dbeta")
    for x, y, what in ((ca, ca2, "ca"), (cb, cb2, "cb"), (cc, cc2, "cc"), (dwp, dwp2, "dwpack"), (dw, dw2, "dw")):
        close(x, y, what)
    assert float(ca2[Cout:].abs().max() if Cout < Cp else 0.0) == 0.0          # padded channels: zero coefficients
