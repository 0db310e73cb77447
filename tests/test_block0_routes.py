"""Block 0's backward route: the plan-time decision (engine.block0_route, host only) against a table written out here, and on the
GPU the kernels each route launches (the labels of a KernelTimer on the engine) against the same table."""
import importlib
import itertools
import os

import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, "soundeventdetection-pytorch_amd", "libsed_hip.so")


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module("soundeventdetection-pytorch_amd")


# C1 mode exists for bf16, 64 mel bins, 32 channels, the dedicated Cin = 1 first layer and SED_C1_MODE not 0; there the route is
# a matter of (block-0 pool, SED_BWD_FUSED):
C1_TABLE = {
    (2, None): "c1_fused",
    (2, "0"): "c1_stats",
    (1, None): "c1_stats",
    (1, "0"): "c1_stats",
}


def test_route_table(sed):
    lib = sed._lib.lib()          # dlopen + the host-only *_supported answers: no GPU
    seen = set()
    for prec, F, ch, pool, c1env, fenv, gf in itertools.product(("bf16", "fp32", "f16x3"), (64, 40), (32, 16), (1, 2), (None, "0"),
                                                                (None, "0"), (False, True)):
        env = {}
        if c1env is not None:
            env["SED_C1_MODE"] = c1env
        if fenv is not None:
            env["SED_BWD_FUSED"] = fenv
        c1 = prec == "bf16" and F == 64 and ch == 32 and c1env is None and not gf
        want = C1_TABLE[(pool, fenv)] if c1 else "z1"
        got = sed.engine.block0_route(lib, prec, F, ch, pool, gf, env)
        assert got == want, (prec, F, ch, pool, env, gf, got, want)
        assert got in sed.engine.C1_ROUTES
        seen.add(got)
    assert seen == set(sed.engine.C1_ROUTES)


# ---- on the GPU: what each route launches for block 0's backward ---------------------------------------------------------------
LAUNCHES = {
    "z1": {"sed_conv3x3_wgrad_fused", "sed_conv3x3_fwd", "sed_bn_bwd_finalize", "sed_conv3x3_c1_gram", "sed_conv3x3_c1_wgrad",
           "sed_sum_partials", "sed_conv3x3_c1_wgrad_combine"},
    "c1_fused": {"sed_conv3x3_bwd_fused_c1", "sed_c1_bwd_tail"},
    "c1_stats": {"sed_conv3x3_wgrad_fused_c1", "sed_conv3x3_dgrad_c1_stats", "sed_c1_bwd_tail"},
    "c1_plain": {"sed_conv3x3_wgrad_fused_c1", "sed_conv3x3_dgrad_c1", "sed_conv3x3_c1_wgrad", "sed_sum_partials",
                 "sed_bn_bwd_finalize_c1", "sed_conv3x3_c1_wgrad_combine", "sed_conv3x3_c1_dgrad"},
}
LAUNCHES["c1_plain_eval"] = (LAUNCHES["c1_plain"] - {"sed_bn_bwd_finalize_c1"}) | {"sed_bn_eval_bwd_finalize_c1", "sed_conv3x3_c1_gram"}

CASES = [  # id, block-0 pool, environment, input gradient, eval mode, plan route, launches
    ("default", 2, {}, False, False, "c1_fused", "c1_fused"),
    ("bwd_fused_0", 2, {"SED_BWD_FUSED": "0"}, False, False, "c1_stats", "c1_stats"),
    ("pool1", 1, {}, False, False, "c1_stats", "c1_stats"),
    ("need_dx", 2, {}, True, False, "c1_fused", "c1_plain"),
    ("eval", 2, {}, True, True, "c1_fused", "c1_plain_eval"),
    ("c1_mode_0", 2, {"SED_C1_MODE": "0"}, False, False, "z1", "z1"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,p0,env,need_dx,evalmode,route,launches", CASES, ids=[c[0] for c in CASES])
def test_block0_backward_launches(sed, monkeypatch, name, p0, env, need_dx, evalmode, route, launches):
    """cfg [(32, p0), (64, 2)], B = 2, T = 12 (three 4-row tiles plus the ragged H + 1 tile of the fused kernel), F = 64, bf16"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sed._lib.lib().sed_config_reload()
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, [(32, p0), (64, 2)], precision="bf16").cuda()
    model.train(not evalmode)
    timer = model.engine.timer = sed.engine.KernelTimer()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 12, 64, generator=g).cuda().requires_grad_(need_dx)
    out = model(x)          # (B, t_out * ratio, 1) logits
    y = (torch.rand(out.shape, generator=g) > 0.7).float().cuda()
    torch.nn.functional.binary_cross_entropy_with_logits(out, y).backward()
    torch.cuda.synchronize()
    plan = next(iter(model.engine._plans.values()))
    assert plan.c1_route == route and plan.c1_mode == (route != "z1")
    assert (plan.c1_mask is not None) == (route == "c1_stats")
    got = {label.partition(":")[0] for label, _, _ in timer.records if label.partition(":")[2].startswith("bwd b0")}
    # in front of every route: pool + ReLU + BN2 backward (its statistics from the pooled tensors where block 1's data gradient left them)
    want = LAUNCHES[launches] | {"sed_pool_relu_bwd_stats_if" if (plan.pool_fused[0] and not evalmode) else "sed_pool_relu_bwd_stats",
                                 "sed_bn_eval_bwd_finalize" if evalmode else "sed_bn_bwd_finalize"}
    assert got == want, (sorted(got - want), sorted(want - got))
    for n, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), n
    if need_dx:
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all()
