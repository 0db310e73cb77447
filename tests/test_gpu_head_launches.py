"""GPU: the launches of one train step per temporal head, label by label.  The full KernelTimer label list -- kernel names AND the
:gru / :sa tags -- of the second FusedTrainer.train_step of four models is compared with the tables below, which were recorded on
the parent of the commit that moved the heads out of CnnEngine into heads.py (from a checkout of that parent, not from this tree):
whoever touches the heads' dispatch sees here which launch moved.  Shape: tests/test_gpu_sa_model.py's step_labels -- CFG =
[(32, 2), (32, 2)], 3 classes, bf16, input (2, 1, 32, 64), t = 8.  The models with attention=True step through the weak ("att", ...)
loss, so the packed route of the event_fc / att_fc backward is the one recorded.  STACK_FWD / STACK_BWD: the conv stack and the
optimizer, the same for every head."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (32, 2)]

STACK_FWD = [
    "sed_pack_conv_weights_batch", "sed_conv3x3_c1_gram:fwd b0c1 1->32 H32 W64", "sed_bn_train_finalize_c1:fwd b0c1 1->32 H32 W64",
    "sed_conv3x3_fwd_c1:fwd b0c2 32->32 H32 W64", "sed_bn_train_finalize:fwd b0c2 32->32 H32 W64", "sed_bn_relu_pool_cnt_fwd:fwd b0",
    "sed_conv3x3_fwd:fwd b1c1 32->32 H16 W32", "sed_bn_train_finalize:fwd b1c1 32->32 H16 W32",
    "sed_conv3x3_fwd:fwd b1c2 32->32 H16 W32", "sed_bn_train_finalize:fwd b1c2 32->32 H16 W32", "sed_bn_relu_pool_fwd:fwd b1",
]
STACK_BWD = [
    "sed_pool_relu_bwd_stats:bwd b1c2 32->32 H16 W32", "sed_bn_bwd_finalize:bwd b1c2 32->32 H16 W32",
    "sed_conv3x3_wgrad_fused:bwd b1c2 32->32 H16 W32", "sed_conv3x3_fwd:bwd b1c2 32->32 H16 W32",
    "sed_bn_bwd_finalize:bwd b1c2 32->32 H16 W32", "sed_conv3x3_wgrad_fused:bwd b1c1 32->32 H16 W32",
    "sed_conv3x3_dgrad_poolstats:bwd b1c1 32->32 H16 W32", "sed_pool_relu_bwd_stats_if:bwd b0c2 32->32 H32 W64",
    "sed_bn_bwd_finalize:bwd b0c2 32->32 H32 W64", "sed_conv3x3_bwd_fused_c1:bwd b0c2 32->32 H32 W64",
    "sed_c1_bwd_tail:bwd b0c1 1->32 H32 W64", "sed_adam_amsgrad_step",
]
FC_ATT = [
    "sed_head_fwd", "sed_att_logits_fwd", "sed_att_loss_fwd_bwd", "sed_att_bwd_pack", "sed_head_bwd", "sed_att_bwd_split",
]
GRU_ATT = [
    "sed_mel_mean_fwd:gru", "sed_gemm_nt:gru", "sed_gemm_nt:gru", "sed_gru_pack_weights:gru", "sed_gru_seq_fwd:gru",
    "sed_head_fwd:gru", "sed_att_logits_fwd:gru", "sed_att_loss_fwd_bwd", "sed_att_bwd_pack:gru", "sed_head_bwd:gru",
    "sed_att_bwd_split:gru", "sed_gru_seq_bwd:gru", "sed_gemm_tn_batch:gru", "sed_transpose_shift:gru", "sed_transpose_shift:gru",
    "sed_gemm_nt:gru", "sed_mel_mean_bwd:gru",
]
SA = [
    "sed_mel_mean_fwd:sa", "sed_gemm_nt:sa", "sed_mhsa_fwd:sa", "sed_gemm_nt:sa", "sed_add_layernorm_fwd:sa", "sed_head_fwd:sa",
    "sed_bce_fwd_bwd", "sed_head_bwd:sa", "sed_add_layernorm_bwd:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa",
    "sed_mhsa_bwd:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_mel_mean_bwd:sa",
]
SA_COMPOSED = [
    "sed_mel_mean_fwd:sa", "sed_gemm_nt:sa", "sed_relpos_expand:sa", "sed_mhsa_fwd_rel:sa", "sed_gemm_nt:sa",
    "sed_add_layernorm_fwd_drop:sa", "sed_gemm_nt:sa", "sed_dwconv_glu_fwd:sa", "sed_bn_train_finalize:sa", "sed_bn_silu_fwd:sa",
    "sed_gemm_nt:sa", "sed_add_layernorm_fwd_drop:sa", "sed_ffn_fwd_drop:sa", "sed_add_layernorm_fwd_drop:sa", "sed_gemm_nt:sa",
    "sed_relpos_expand:sa", "sed_mhsa_fwd_rel:sa", "sed_gemm_nt:sa", "sed_add_layernorm_fwd_drop:sa", "sed_gemm_nt:sa",
    "sed_dwconv_glu_fwd:sa", "sed_bn_train_finalize:sa", "sed_bn_silu_fwd:sa", "sed_gemm_nt:sa", "sed_add_layernorm_fwd_drop:sa",
    "sed_ffn_fwd_drop:sa", "sed_add_layernorm_fwd_drop:sa", "sed_head_fwd:sa", "sed_att_logits_fwd:sa", "sed_att_loss_fwd_bwd",
    "sed_att_bwd_pack:sa", "sed_head_bwd:sa", "sed_att_bwd_split:sa", "sed_add_layernorm_bwd_drop:sa", "sed_transpose_shift:sa",
    "sed_gemm_nt:sa", "sed_ffn_act_bwd_drop:sa", "sed_gemm_tn:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa",
    "sed_add_layernorm_bwd_drop:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_gemm_tn:sa", "sed_bn_silu_bwd_reduce:sa",
    "sed_bn_bwd_finalize:sa", "sed_dwconv_glu_bwd:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa",
    "sed_add_layernorm_bwd_drop:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_mhsa_bwd_rel:sa",
    "sed_relpos_fold:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_add_layernorm_bwd_drop:sa",
    "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_ffn_act_bwd_drop:sa", "sed_gemm_tn:sa", "sed_gemm_tn:sa",
    "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_add_layernorm_bwd_drop:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa",
    "sed_gemm_tn:sa", "sed_bn_silu_bwd_reduce:sa", "sed_bn_bwd_finalize:sa", "sed_dwconv_glu_bwd:sa", "sed_gemm_tn:sa",
    "sed_transpose_shift:sa", "sed_gemm_nt:sa", "sed_add_layernorm_bwd_drop:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa",
    "sed_gemm_nt:sa", "sed_mhsa_bwd_rel:sa", "sed_relpos_fold:sa", "sed_gemm_tn:sa", "sed_transpose_shift:sa", "sed_gemm_nt:sa",
    "sed_mel_mean_bwd:sa",
]
COMPOSED = dict(sa_heads=1, sa_layers=2, sa_ffn=64, sa_conv_kernel=3, sa_dropout=0.1, sa_dropout_seed=5, sa_window=(2, None), sa_rel_pos=3,
                attention=True)
MODELS = {
    "fc_att": (lambda sed: sed.Cnn_AvgPooling(3, CFG, precision="bf16", attention=True), FC_ATT, None),
    "gru_att": (lambda sed: sed.Crnn_AvgPooling(3, CFG, precision="bf16", gru_hidden=32, attention=True), GRU_ATT, "gru"),
    "sa": (lambda sed: sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1), SA, "sa"),
    "sa_composed": (lambda sed: sed.Csa_AvgPooling(3, CFG, precision="bf16", **COMPOSED), SA_COMPOSED, "sa"),
}


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.mark.parametrize("name", list(MODELS))
def test_second_step_launches_the_recorded_labels(sed, name):
    build, head_labels, plan_field = MODELS[name]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 32, 64, generator=g).cuda()
    y = torch.zeros(2, 32, 3, device="cuda")
    y[0, 4:13, 0] = 1.0
    torch.manual_seed(0)
    mdl = build(sed).cuda()
    weak = dict(weak_pooling="att", weak_only=True) if mdl.attention else {}
    tr = sed.FusedTrainer(mdl, lr=1e-3, recall_factor=5.0, **weak)
    tr.train_step(x, y)             # (first step: allocations)
    mdl.engine.timer = sed.engine.KernelTimer()
    tr.train_step(x, y)
    torch.cuda.synchronize()
    got = [label for label, _, _ in mdl.engine.timer.records]
    want = STACK_FWD + head_labels + STACK_BWD
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5] + [len(got), len(want)]
    (plan,) = mdl.engine._plans.values()
    assert plan.att_pending == bool(mdl.attention)
    assert (plan.sa is not None) == (plan_field == "sa") and (plan.gru is not None) == (plan_field == "gru")
    for n, grad in tr.flat.G.items():
        assert bool(torch.isfinite(grad).all()), n
