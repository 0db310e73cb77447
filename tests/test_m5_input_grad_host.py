"""CPU-side checks of M5's input-gradient / eval-mode backward feature (no GPU needed)."""
import importlib
from types import SimpleNamespace

import pytest

PKG = "soundeventdetection-pytorch_amd"


def test_m5_engine_refuses_eval_backward_without_a_kept_forward():
    eng_mod = importlib.import_module(PKG + ".m5_engine")
    plan = SimpleNamespace(trained=False, keep=False)
    eng = eng_mod.M5Engine.__new__(eng_mod.M5Engine)
    with pytest.raises(RuntimeError, match="eval-mode"):
        eng_mod.M5Engine.backward(eng, plan, {}, {})


def test_m5_function_backward_of_an_unkept_eval_forward_names_the_cause():
    wm = importlib.import_module(PKG + ".models.waveform_models")
    ctx = SimpleNamespace(model=SimpleNamespace(_fwd_serial=1), serial=1, training=False, plan=None, keep=False)
    with pytest.raises(RuntimeError, match="eval-mode"):
        wm._M5Function.backward(ctx, None)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_waveform_training_refuses_x3_precision_before_the_dataset(tmp_path, precision):
    main = importlib.import_module(PKG + ".main")
    missing = str(tmp_path / "no_such_dataset_dir")
    argv = ["--train_features", "Waveform", "--dataset_name", "TAU", "--dataset_dir", missing, "--precision", precision]
    with pytest.raises(ValueError, match=r"bf16.*fp32") as ei:
        main.main(argv)
    assert "Waveform" in str(ei.value) and precision in str(ei.value)


def test_supported_combinations_pass_validation():
    main = importlib.import_module(PKG + ".main")
    for argv in (["--train_features", "Waveform", "--precision", "bf16"], ["--train_features", "Waveform", "--precision", "fp32"],
                 ["--train_features", "Spectogram", "--precision", "f16x3"]):
        main.validate_args(main.build_parser().parse_args(argv))
