"""conv_block1's route of the raw-waveform M5: the plan-time decision (m5_engine.conv1_route, host only) against a table written out
here, and on the GPU the kernels each route launches (the labels of a KernelTimer on the engine) against a table per case."""
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


# (precision, SED_M5_MFMA, SED_M5_FWD2, SED_M5_POOLSTATS) -> (route, fwd2, poolstats); None = unset
ROUTE_TABLE = {
    ("bf16", None, None, None): ("mfma", True, True),
    ("bf16", None, None, "0"): ("mfma", True, False),
    ("bf16", None, "0", None): ("mfma", False, True),
    ("bf16", None, "0", "0"): ("mfma", False, False),
    ("bf16", "0", None, None): ("valu", False, False),
    ("bf16", "0", None, "0"): ("valu", False, False),
    ("bf16", "0", "0", None): ("valu", False, False),
    ("bf16", "0", "0", "0"): ("valu", False, False),
    ("fp32", None, None, None): ("valu", False, False),
    ("fp32", None, None, "0"): ("valu", False, False),
    ("fp32", None, "0", None): ("valu", False, False),
    ("fp32", None, "0", "0"): ("valu", False, False),
    ("fp32", "0", None, None): ("valu", False, False),
    ("fp32", "0", None, "0"): ("valu", False, False),
    ("fp32", "0", "0", None): ("valu", False, False),
    ("fp32", "0", "0", "0"): ("valu", False, False),
}


def test_route_table(sed):
    lib = sed._lib.lib()          # dlopen + the host-only sed_m5_fwd2_supported answer: no GPU
    route_of = sed.m5_engine.conv1_route
    seen = set()
    for prec, mfma, fwd2, pst in itertools.product(("bf16", "fp32"), (None, "0"), (None, "0"), (None, "0")):
        env = {k: v for k, v in (("SED_M5_MFMA", mfma), ("SED_M5_FWD2", fwd2), ("SED_M5_POOLSTATS", pst)) if v is not None}
        got = route_of(lib, prec, env)
        assert got == ROUTE_TABLE[(prec, mfma, fwd2, pst)], (prec, env, got)
        assert got[0] in sed.m5_engine.CONV1_ROUTES
        seen.add(got[0])
    assert seen == set(sed.m5_engine.CONV1_ROUTES) and len(ROUTE_TABLE) == 16


# ---- on the GPU: what each route launches for conv_block1 ------------------------------------------------------------------------
FWD = {
    "two_pass": {"sed_m5_conv1_stats", "sed_bn_train_finalize", "sed_m5_conv1_bn_relu_pool_fwd"},
    "one_pass": {"sed_m5_conv1_fwd", "sed_bn_train_finalize", "sed_bn_relu_maxpool4_fwd"},
    "two_pass_eval_kept": {"sed_bn_eval_coeffs", "sed_bn_eval_stats", "sed_m5_conv1_bn_relu_pool_fwd"},
}
_MFMA_DW = {"sed_m5_conv1_wgrad_fused_pool", "sed_sum_partials"}
BWD = {
    "mfma_pooled_stats": {"sed_maxpool4_pooled_stats", "sed_maxpool4_relu_bwd_if", "sed_bn_bwd_finalize"} | _MFMA_DW,
    "mfma_z_stats": {"sed_maxpool4_relu_bwd", "sed_bn_bwd_finalize"} | _MFMA_DW,
    "mfma_eval": {"sed_maxpool4_relu_bwd", "sed_bn_eval_bwd_finalize"} | _MFMA_DW,
    "valu": {"sed_maxpool4_relu_bwd", "sed_bn_bwd_finalize", "sed_bn_bwd_apply", "sed_m5_conv1_wgrad", "sed_sum_partials"},
}
BWD["mfma_pooled_stats_dx"] = BWD["mfma_pooled_stats"] | {"sed_m5_conv1_dgrad_fused_pool"}

CASES = [  # id, precision, environment, input gradient, eval mode, plan (route, fwd2, poolstats), forward launches, backward launches
    ("default", "bf16", {}, False, False, ("mfma", True, True), "two_pass", "mfma_pooled_stats"),
    ("poolstats_0", "bf16", {"SED_M5_POOLSTATS": "0"}, False, False, ("mfma", True, False), "two_pass", "mfma_z_stats"),
    ("fwd2_0", "bf16", {"SED_M5_FWD2": "0"}, False, False, ("mfma", False, True), "one_pass", "mfma_pooled_stats"),
    ("mfma_0", "bf16", {"SED_M5_MFMA": "0"}, False, False, ("valu", False, False), "one_pass", "valu"),
    ("fp32", "fp32", {}, False, False, ("valu", False, False), "one_pass", "valu"),
    ("need_dx", "bf16", {}, True, False, ("mfma", True, True), "two_pass", "mfma_pooled_stats_dx"),
    ("eval_kept", "bf16", {}, False, True, ("mfma", True, True), "two_pass_eval_kept", "mfma_eval"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec,env,need_dx,evalmode,route,fwd,bwd", CASES, ids=[c[0] for c in CASES])
def test_conv_block1_launches(sed, monkeypatch, name, prec, env, need_dx, evalmode, route, fwd, bwd):
    """M5(1) at B = 8, L = 1111: conv1 length 278 = two full 128-step tiles and a ragged one, then 69 -> 17 -> 4 -> 1 through the
    pools (the smallest frame the pool stack accepts with more than one tile)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sed._lib.lib().sed_config_reload()
    torch.manual_seed(0)
    model = sed.M5(1, precision=prec).cuda()          # a fresh engine: the knobs take effect when its plan is built
    model.train(not evalmode)
    timer = model.engine.timer = sed.engine.KernelTimer()
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn(8, 1, 1111, generator=g)).cuda().requires_grad_(need_dx)
    out = model(x)          # (B, 1) logits; in eval mode kept for the backward (grad mode on, parameters require grad)
    y = (torch.rand(out.shape, generator=g) > 0.6).float().cuda()
    torch.nn.functional.binary_cross_entropy_with_logits(out, y).backward()
    torch.cuda.synchronize()
    plan = next(iter(model.engine._plans.values()))
    assert (plan.route, plan.fwd2, plan.poolstats) == route
    assert [ly.H for ly in plan.layers if ly.first] == [278] and plan.t_out == 1
    got = {"fwd": set(), "bwd": set()}
    for label, _, _ in timer.records:
        kernel, _, tag = label.partition(":")
        if tag[4:].startswith("conv_block1."):
            got[tag[:3]].add(kernel)
    assert got["fwd"] == FWD[fwd], (sorted(got["fwd"] - FWD[fwd]), sorted(FWD[fwd] - got["fwd"]))
    assert got["bwd"] == BWD[bwd], (sorted(got["bwd"] - BWD[bwd]), sorted(BWD[bwd] - got["bwd"]))
    for n, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), n
    if need_dx:
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all()
