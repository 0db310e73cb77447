"""Host side of the mel-bin width setting (no GPU): the mel_bins keyword, the CLI flags, model_description, the plan-time
ValueErrors raised before any launch, and the width-general sizing helpers of libsed_hip.so."""
import importlib
import pickle

import numpy as np
import pytest

PKG = "soundeventdetection-pytorch_amd"
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


def test_mel_bins_keyword_and_description(sed, capsys):
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32", mel_bins=40)
    assert m.mel_bins == 40 and m.engine.mel_bins == 40
    m.model_description()
    out = capsys.readouterr().out
    assert "Input: (b, 1, 181, 40)" in out and "conv_block -> (b, 128, 22, 5)" in out
    assert sed.Cnn_AvgPooling(1, MAIN_CFG).mel_bins is None
    c = importlib.import_module(PKG + ".models.spectogram_models").Crnn_AvgPooling(1, MAIN_CFG, gru_hidden=32, mel_bins=96)
    assert c.engine.mel_bins == 96 and c.engine.head == "gru"
    # the parameters do not depend on the width: a checkpoint of one width loads into a model of another
    m64 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32")
    sd = m64.state_dict()
    assert {k: v.shape for k, v in sd.items()} == {k: v.shape for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    for bad in (0, -3, 2.5, "40", True):
        with pytest.raises(ValueError):
            sed.Cnn_AvgPooling(1, MAIN_CFG, mel_bins=bad)


def test_plan_time_errors_before_any_launch(sed):
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=40)
    with pytest.raises(ValueError, match="differs from the declared"):
        m.engine.plan(2, 30, 64, "cpu")
    with pytest.raises(ValueError, match="unsupported"):
        sed.Cnn_AvgPooling(1, MAIN_CFG, mel_bins=300).engine.plan(2, 30, 300, "cpu")
    with pytest.raises(ValueError, match="pooling stack"):
        sed.Cnn_AvgPooling(1, MAIN_CFG, mel_bins=3).engine.plan(2, 30, 3, "cpu")
    # undeclared: today's refusal
    with pytest.raises(ValueError, match="need 8/16/32/64"):
        sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32").engine.plan(2, 30, 48, "cpu")


def test_plan_layers_at_uncovered_widths(sed):
    """a declared 128-bin f16x3 model: block 0 (W = 128) packs and runs in exact fp32, the others keep the split-operand dtype"""
    L = sed._lib
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="f16x3", mel_bins=128)
    p = m.engine.plan(1, 24, 128, "cpu")
    assert [ly.W for ly in (b[0] for b in p.layers)] == [128, 64, 32, 16]
    assert [b[1].dt_mm for b in p.layers] == [L.SED_F32, L.SED_F32H3, L.SED_F32H3, L.SED_F32H3]
    assert not p.c1_mode and not any(f for b in p.bwd_fused for f in b)
    assert m.engine._grad_dtype(1, 24, 128) == L.SED_F32                 # no fp16 pre-scale exponent at a general width
    assert m.engine._grad_dtype(1, 24, 64) & 0xff == L.SED_F32H3
    p40 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=40).engine.plan(2, 30, 40, "cpu")
    assert [b[0].W for b in p40.layers] == [40, 20, 10, 5] and p40.w_out == 5


def test_sizing_helpers(sed):
    lib = sed._lib.lib()
    # the values before width-general kernels existed (the formulas of the specialised kernels), at the covered widths
    for (B, H, W, ci, co) in [(32, 6001, 64, 32, 32), (32, 3000, 32, 32, 64), (32, 1500, 16, 64, 128), (32, 750, 8, 128, 128),
                              (2, 37, 64, 32, 32), (4, 9, 8, 256, 512)]:
        assert lib.sed_conv_nparts(B, H, W) == min(B * -(-H * W // 256), 1024)
        assert lib.sed_pool_bwd_nparts(B, H, W, co) == min(max(B * H, 1), 1024)
    assert lib.sed_conv_wgrad_ws_floats(32, 6001, 64, 32, 32) == 1024 * 9 * 32 * 32
    for W in (8, 16, 32, 64):
        n = lib.sed_conv_wgrad_ws_floats(2, 37, W, 64, 64)
        assert n > 0 and n % (9 * 64 * 64) == 0
    for W in (1, 5, 40, 100, 128, 200, 256):
        for (ci, co) in [(32, 32), (64, 128), (128, 64)]:
            n = lib.sed_conv_wgrad_ws_floats(2, 37, W, ci, co)
            assert 0 < n < 2 ** 40 and n % (9 * ci * co) == 0
            assert 0 < lib.sed_conv_nparts(2, 37, W) <= 1024
            assert 0 < lib.sed_pool_bwd_nparts(2, 37, W, co) <= 1024


def test_cli_flags(tmp_path):
    main = importlib.import_module(PKG + ".main")
    infer = importlib.import_module(PKG + ".infer")
    assert main.build_parser().parse_args([]).mel_bins is None
    assert main.build_parser().parse_args(["--mel_bins", "40"]).mel_bins == 40
    assert infer.build_parser().parse_args(["a.wav", "--ckpt", "c", "--mel_bins", "96"]).mel_bins == 96
    p = tmp_path / "ms.pkl"
    with open(p, "wb") as f:
        pickle.dump({"mean": np.zeros(64, np.float32), "std": np.ones(64, np.float32)}, f)
    mean, std = infer.load_mean_std(str(p), 64)
    assert len(mean) == 64 and len(std) == 64
    with pytest.raises(ValueError, match="64 entries"):
        infer.load_mean_std(str(p), 40)
    with pytest.raises(ValueError, match="64 entries"):      # checked before the GPU is needed
        infer.infer_file("missing.wav", "missing.ckpt", mean_std=str(p), mel_bins=40)


def test_main_builds_the_declared_config(monkeypatch):
    """main.py: the config (front-end, dataset, synthetic data) and the model take --mel_bins"""
    main = importlib.import_module(PKG + ".main")
    import torch
    seen = {}
    syn = importlib.import_module(PKG + ".dataset.synthetic")

    class Probe(syn.SyntheticSedDataset):
        def __init__(self, *a, **k):
            seen["mel_bins"] = k.get("mel_bins")
            super().__init__(*a, **k)
    monkeypatch.setattr(syn, "SyntheticSedDataset", Probe)
    args = main.build_parser().parse_args(["--dataset_name", "synthetic", "--mel_bins", "40", "--batch_size", "4",
                                           "--precision", "fp32"])
    dataset, model, _, desc = main.get_spectogram_dataset_model_and_criterion(args, torch.device("cpu"))
    assert seen["mel_bins"] == 40 and model.mel_bins == 40 and "_Mel-40_" in desc
    x, _ = dataset[0]
    assert x.shape[-1] == 40
