"""CPU tests of the grouped optimizer's host side: tests/optim_formula.py (the float64 definition the GPU tests gate the kernels with)
against torch.optim.Adam / AdamW with real param_groups and against LambdaLR, mutants the comparison has to reject, the selectors,
the tile table and its validation, the option refusals, the command-line flags and the state_dict layout."""
import importlib
import math

import numpy as np
import pytest
import torch

import optim_formula as F

PKG = "soundeventdetection-pytorch_amd"
SIZES = [1, 3, 4, 5, 4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1, 8 * 1024 + 4]
SCHEDULES = [dict(kind="const"), dict(kind="step", every=3, gamma=0.5), dict(kind="cosine", total=9, floor=0.1),
             dict(kind="linear", total=9, floor=0.25), dict(kind="invsqrt")]


@pytest.fixture(scope="module")
def tr():
    return importlib.import_module(PKG + ".train")


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [0, 1, 3])
@pytest.mark.parametrize("kw", SCHEDULES, ids=[s["kind"] for s in SCHEDULES])
def test_schedule_against_lambda_lr(tr, kw, warmup):
    """LambdaLR multiplies the initial rate by the factor of the epoch counter, which is s - 1 for the s-th optimizer step."""
    base = 3e-3
    kind = kw["kind"]
    every, gamma, total, floor = kw.get("every", 200), kw.get("gamma", 0.997), kw.get("total", 0), kw.get("floor", 0.0)

    def factor(epoch):
        s = epoch + 1
        w = min(1.0, s / warmup) if warmup else 1.0
        u = min(1.0, max(0.0, (s - warmup) / (total - warmup))) if total else 0.0
        d = {"const": 1.0, "step": gamma ** ((s - 1) // every), "cosine": floor + (1 - floor) * 0.5 * (1 + math.cos(math.pi * u)),
             "linear": floor + (1 - floor) * (1 - u), "invsqrt": math.sqrt(max(warmup, 1) / max(s, warmup, 1))}[kind]
        return w * d

    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=base)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, factor)
    sched = tr.LRSchedule(warmup=warmup, **kw)
    for s in range(1, 25):
        want = opt.param_groups[0]["lr"]
        for got in (F.lr_at(base, s, kind, warmup, total, every, gamma, floor), tr.lr_at(base, s, sched)):
            assert got == pytest.approx(want, rel=1e-14, abs=0.0), (kind, warmup, s)
        opt.step()
        lam.step()
    if kind in ("cosine", "linear"):
        assert F.lr_at(base, total, kind, warmup, total, floor=floor) == pytest.approx(base * floor, rel=1e-12)
        assert F.lr_at(base, total + 50, kind, warmup, total, floor=floor) == pytest.approx(base * floor, rel=1e-12)
    if warmup:
        assert F.lr_at(base, warmup, kind, warmup, total or 99, every, gamma, floor) == pytest.approx(
            base * factor(warmup - 1), rel=1e-14)
        assert F.lr_at(base, 1, "const", warmup) == pytest.approx(base / warmup, rel=1e-15)


def test_schedule_validation(tr):
    ok = tr.LRSchedule("cosine", warmup=3, total=8, floor=0.5)
    assert ok.as_dict() == dict(kind="cosine", warmup=3, total=8, every=200, gamma=0.997, floor=0.5)
    ref = tr.LRSchedule("step")
    assert (ref.every, ref.gamma) == (tr.LR_DECAY_FREQ, tr.LR_DECAY) == (200, 0.997)
    bad = [dict(kind="poly"), dict(kind="const", warmup=-1), dict(kind="const", warmup=1.5), dict(kind="const", warmup=True),
           dict(kind="cosine", warmup=3, total=3), dict(kind="linear", total=0), dict(kind="step", every=0),
           dict(kind="const", floor=-0.1), dict(kind="const", floor=1.1), dict(kind="const", floor=float("nan")),
           dict(kind="step", gamma=0.0), dict(kind="step", gamma=float("inf")), dict(kind="step", gamma=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            tr.LRSchedule(**kw)
    with pytest.raises(ValueError):
        tr.lr_at(1e-3, 0, ok)


# ---- the step against torch.optim with real param_groups -------------------------------------------------------------------------
SPECS = [(1.0, 1e-2, False), (0.1, 0.0, False), (2.5, 3e-2, False), (1.0, 1e-2, True)]
SHAPES = [(5,), (3, 4), (7,), (2, 3), (6,), (4,), (1,), (9,)]
GROUP_OF_PARAM = [0, 1, 2, 3, 1, 0, 3, 2]


def _torch_run(decoupled, amsgrad, steps, sched, base, max_norm, seed=0):
    """(per-step flat gradients, per-step (p, m, v, vmax), norms) from torch.optim on float64 parameters in 4 groups"""
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in SHAPES]
    groups = [{"params": [p for p, k in zip(params, GROUP_OF_PARAM) if k == gi], "weight_decay": SPECS[gi][1]} for gi in range(4)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=base, amsgrad=amsgrad, foreach=False)
    hist = []
    for s in range(1, steps + 1):
        before = [p.detach().clone() for p in params]
        grads = [torch.randn(p.shape, generator=g, dtype=torch.float64) * (2.0 if s < 3 else 0.05) for p in params]
        for p, gr, k in zip(params, grads, GROUP_OF_PARAM):
            p.grad = None if SPECS[k][2] else gr.clone()                  # a frozen parameter has no gradient
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = F.lr_at(base, s, **sched) * SPECS[gi][0]
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)) if max_norm else None
        opt.step()
        st = [{k: t.clone() for k, t in opt.state.get(p, {}).items()} for p in params]      # (torch updates them in place)
        hist.append((before, grads, [p.detach().clone() for p in params], st, norm))
    return params, opt, hist


def _flat(ts):
    return np.concatenate([np.asarray(t.detach().reshape(-1)) for t in ts])


def _formula_run(decoupled, amsgrad, steps, sched, base, max_norm, mutant=None):
    """the same run through optim_formula; returns the worst relative deviation from torch over p, m, v, vmax and the norm"""
    params, opt, hist = _torch_run(decoupled, amsgrad, steps, sched, base, max_norm)
    elem_group = np.concatenate([np.full(int(np.prod(s)), k) for s, k in zip(SHAPES, GROUP_OF_PARAM)])
    n = elem_group.size
    p = _flat(hist[0][0])
    m, v, x = np.zeros(n), np.zeros(n), (np.zeros(n) if amsgrad else None)
    worst = 0.0

    def dev(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))

    sched_m, specs = dict(sched), list(SPECS)
    for s, (before, grads, after, st, tnorm) in enumerate(hist, start=1):
        g = _flat(grads)
        g_seen = g.copy()
        if mutant == "nan_in_frozen":
            g_seen[np.asarray([SPECS[k][2] for k in elem_group])] = np.nan      # not a mutant: the formula must not look there
        lr = F.lr_at(base, s + 1 if mutant == "warmup_off_by_one" else s, **sched_m)
        if mutant == "cosine_without_floor":
            lr = F.lr_at(base, s, **dict(sched_m, floor=0.0))
        coef = 1.0
        if max_norm:
            norm = F.grouped_norm(g_seen, elem_group, [(a, b, False) for a, b, _ in specs] if mutant == "norm_with_frozen" else specs)
            worst = max(worst, abs(norm - tnorm) / tnorm)
            coef = F.clip_coef(norm, max_norm)
        use = specs
        if mutant == "decay_on_wd0":
            use = [(a, b if b else 1e-2, c) for a, b, c in specs]
        p, m1, v, x = F.grouped_adam_step(p, g_seen, m, v, x, elem_group, use, lr, s, decoupled=decoupled, coef=coef)
        if mutant == "frozen_updates_m":
            fz = np.asarray([SPECS[k][2] for k in elem_group])
            m1 = np.where(fz, m + 0.1 * (g - m), m1)
        m = m1
        zeros = [torch.zeros(sh, dtype=torch.float64) for sh in SHAPES]
        tm = _flat([q.get("exp_avg", z) for q, z in zip(st, zeros)])
        tv = _flat([q.get("exp_avg_sq", z) for q, z in zip(st, zeros)])
        worst = max(worst, dev(p, _flat(after)), float(np.max(np.abs(m - tm))) / max(float(np.max(np.abs(tm))), 1e-300),
                    float(np.max(np.abs(v - tv))) / max(float(np.max(np.abs(tv))), 1e-300))
        if amsgrad:
            tx = _flat([q.get("max_exp_avg_sq", z) for q, z in zip(st, zeros)])
            worst = max(worst, float(np.max(np.abs(x - tx))) / max(float(np.max(np.abs(tx))), 1e-300))
    frozen_params = [i for i, k in enumerate(GROUP_OF_PARAM) if SPECS[k][2]]
    assert all(not hist[-1][3][i] for i in frozen_params), "torch keeps no state for a parameter without a gradient"
    return worst


COSINE = dict(kind="cosine", warmup=3, total=10, floor=0.2)


@pytest.mark.parametrize("amsgrad", [True, False], ids=["amsgrad", "plain"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_formula_against_torch_param_groups(decoupled, amsgrad):
    for max_norm in (None, 0.75):
        assert _formula_run(decoupled, amsgrad, 12, COSINE, 2e-2, max_norm) <= 1e-12
        assert _formula_run(decoupled, amsgrad, 12, COSINE, 2e-2, max_norm, mutant="nan_in_frozen") <= 1e-12
    assert _formula_run(decoupled, amsgrad, 12, dict(kind="step", every=4, gamma=0.5), 2e-2, None) <= 1e-12


@pytest.mark.parametrize("mutant", ["warmup_off_by_one", "cosine_without_floor", "decay_on_wd0", "frozen_updates_m",
                                    "norm_with_frozen"])
def test_the_comparison_rejects_mutants(mutant):
    """each of these passes a sloppier check: the 1e-12 gate against torch must not"""
    max_norm = 0.75 if mutant == "norm_with_frozen" else None
    assert _formula_run(True, True, 12, COSINE, 2e-2, max_norm, mutant=mutant) > 1e-6, mutant


# ---- selectors and groups --------------------------------------------------------------------------------------------------------
def test_selectors(tr):
    names = [f"conv_blocks.{i}.conv1.weight" for i in (0, 1, 10)] + ["conv_blocks.1.bn1.bias", "event_fc.weight", "event_fc.bias"]
    hit = [n for n in names if tr.selector_matches(["conv_blocks.1"], n)]
    assert hit == ["conv_blocks.1.conv1.weight", "conv_blocks.1.bn1.bias"], "conv_blocks.1 must not take conv_blocks.10"
    assert tr.selector_matches(["event_fc.weight"], "event_fc.weight") and not tr.selector_matches(["event_fc.w"], "event_fc.weight")
    assert tr.selector_matches(["conv_blocks."], "conv_blocks.0.conv1.weight")
    specs, asg = tr.resolve_param_groups(names, [{"params": ["conv_blocks.1"], "frozen": True},
                                                 {"params": ["conv_blocks"], "lr_scale": 0.5, "weight_decay": 0.0},
                                                 {"params": lambda n: n.endswith(".bias"), "lr_scale": 2.0}], weight_decay=0.25)
    assert asg == [2, 1, 2, 1, 0, 3], "the first match wins; the unmatched remainder is group 0"
    assert specs == [(1.0, 0.25, False), (1.0, 0.25, True), (0.5, 0.0, False), (2.0, 0.25, False)], "weight_decay None inherits"
    assert tr.resolve_param_groups(names, None, 0.5) == ([(1.0, 0.5, False)], [0] * 6)
    bad = [[{"params": ["nothing"]}], [{"params": ["conv_blocks"]}, {"params": ["conv_blocks.1"]}],
           [{"params": ["event_fc"], "lr_scale": -1.0}], [{"params": ["event_fc"], "lr_scale": float("inf")}],
           [{"params": ["event_fc"], "weight_decay": -1e-3}], [{"params": ["event_fc"], "weight_decay": float("nan")}],
           [{"params": ["conv_blocks", "event_fc"], "frozen": True}], [{"params": "event_fc"}], [{"lr_scale": 1.0}],
           [{"params": ["event_fc"], "lr": 1.0}], [{"params": [n]} for n in names] * 11]
    for groups in bad:
        with pytest.raises(ValueError):
            tr.resolve_param_groups(names, groups)
    assert len(tr.resolve_param_groups([f"p{i}" for i in range(63)], [{"params": [f"p{i}"]} for i in range(63)])[0]) == 64
    with pytest.raises(ValueError, match="64"):
        tr.resolve_param_groups([f"p{i}" for i in range(64)], [{"params": [f"p{i}"]} for i in range(64)])


def test_refusals_come_before_the_model_is_touched(tr):
    class Named:
        """a model that has names only: anything else means the constructor went past validation"""
        def named_parameters(self):
            return iter([("a.weight", None), ("a.bias", None)])

        def __getattr__(self, name):
            raise AssertionError(f"model.{name} touched before the options were validated")

    for kw in (dict(param_groups=[{"params": ["b"]}]), dict(param_groups=[{"params": ["a"], "frozen": True}]),
               dict(param_groups=[{"params": ["a"], "lr_scale": float("nan")}]), dict(lr_schedule=tr.LRSchedule("const"), lr=float("inf"))):
        kw.setdefault("lr", 1e-3)
        with pytest.raises(ValueError):
            tr.FusedTrainer(Named(), **kw)
    with pytest.raises(TypeError):
        tr.FusedTrainer(Named(), 1e-3, lr_schedule="cosine")
    assert tr.check_group_options(Named(), 1e-3) is None


def test_no_decay_groups_on_a_conformer_model(sed, tr):
    torch.manual_seed(0)
    m = sed.Csa_AvgPooling(3, [(32, 2), (32, 2)], precision="fp32", sa_heads=1, mel_bins=8, sa_layers=2, sa_ffn=96, sa_conv_kernel=5,
                           sa_norm_first=True, sa_macaron=True)
    groups = tr.no_decay_groups(m)
    specs, asg = tr.resolve_param_groups([n for n, _ in m.named_parameters()], groups, weight_decay=0.05)
    assert specs == [(1.0, float(np.float32(0.05)), False), (1.0, 0.0, False)]
    seen = {0: 0, 1: 0}
    for (n, p), g in zip(m.named_parameters(), asg):
        assert g == (1 if p.ndim <= 1 else 0), n
        seen[g] += 1
        if "norm" in n or ".bn" in n or n.endswith("bias"):
            assert g == 1, f"{n} must not be decayed"
    assert seen[0] > 0 and seen[1] > 0
    assert any("norm" in n for n, _ in m.named_parameters())


# ---- tiles -----------------------------------------------------------------------------------------------------------------------
def _layout(tr):
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(k)) for k in SIZES])
    return tr.FlatParams(m)


def test_build_tiles(tr):
    assert tr.TILE4 == 1024 and tr.MAX_GROUPS == 64
    lib = importlib.import_module(PKG + "._lib")
    assert lib.lib().sed_opt_tile4() == tr.TILE4
    flat = _layout(tr)
    asg = [0, 1, 2, 3, 0, 1, 2, 3]
    specs = [(1.0, 0.01, False), (0.1, 0.0, False), (2.5, 0.03, False), (1.0, 0.0, True)]
    tiles, groups = tr.build_tiles(flat, asg, specs)
    assert tiles.dtype == np.int32 and groups.dtype == np.float32 and groups.shape == (4, 4)
    want = []
    for n, g in zip(flat.names, asg):
        s4, c4 = flat.offsets[n] // 4, (flat.P[n].numel() + 3) // 4
        want += [(s4 + o, min(1024, c4 - o), g, 0) for o in range(0, c4, 1024)]
    assert tiles.tolist() == [list(w) for w in want]
    assert [c for _, c, _, _ in want] == [1, 1, 1, 2, 1024, 1024, 1024, 1, 1024, 1024, 1]
    assert int(tiles[:, 1].sum()) * 4 == flat.numel and int(tiles[:, 1].max()) <= tr.TILE4
    assert groups.tolist() == [[np.float32(a), np.float32(b), 1.0 if c else 0.0, 0.0] for a, b, c in specs]
    t1, g1 = tr.build_tiles(flat, [0] * 8)
    assert g1.tolist() == [[1.0, 0.0, 0.0, 0.0]] and set(t1[:, 2].tolist()) == {0}
    for bad_asg, bad_specs in (([0] * 7, specs), ([0, 1, 2, 4, 0, 1, 2, 3], specs), ([-1] + [0] * 7, specs), ([0] * 8, []),
                               ([0] * 8, [(1.0, 0.0, False)] * 65)):
        with pytest.raises(ValueError):
            tr.build_tiles(flat, bad_asg, bad_specs)

    def corrupt(fn, match):
        t, g = tiles.copy(), groups.copy()
        out = fn(t, g)
        t, g = out if out is not None else (t, g)
        with pytest.raises(ValueError, match=match):
            tr.check_tiles(t, g, flat, asg)

    tr.check_tiles(tiles, groups, flat, asg)
    corrupt(lambda t, g: (t[:-1], g), "cover")                            # the last float4 uncovered
    corrupt(lambda t, g: (t[1:], g), "expected 0")                        # the first
    corrupt(lambda t, g: t.__setitem__((4, 1), 1023), "expected")         # a gap
    corrupt(lambda t, g: t.__setitem__((4, 0), 4), "expected")            # an overlap
    corrupt(lambda t, g: (np.concatenate([t[:5], t[4:]]), g), "expected")  # not ascending
    corrupt(lambda t, g: (np.concatenate([t[:2], [[2, 3, 2, 0]], t[4:]]).astype(np.int32), g), "crosses")   # parameters 2 and 3 merged
    corrupt(lambda t, g: (np.concatenate([t[:4], [[5, 2048, 0, 0]], t[6:]]).astype(np.int32), g), "count4")
    corrupt(lambda t, g: t.__setitem__((0, 1), 0), "count4")
    corrupt(lambda t, g: t.__setitem__((5, 2), 2), "group")               # a tile in another parameter's group
    corrupt(lambda t, g: t.__setitem__((3, 3), 7), "fourth")
    corrupt(lambda t, g: (t.astype(np.int64), g), "int32")
    corrupt(lambda t, g: (t, g[:3]), "outside the group table")
    corrupt(lambda t, g: (t, g.astype(np.float64)), "float32")


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_cli_flags(sed, tr):
    main = importlib.import_module(PKG + ".main")
    parse = main.build_full_parser().parse_args
    a = parse([])
    assert (a.lr_schedule, a.warmup_steps, a.lr_total_steps, a.lr_floor, a.no_decay_norm_bias, a.freeze, a.lr_scale) == (
        "reference", 0, None, 0.0, False, None, None)
    assert main.schedule_options(a) == {}, "the defaults are today's path: no keyword reaches train()"
    main.validate_args(a)
    a = parse(["--lr_schedule", "cosine", "--warmup_steps", "500", "--lr_floor", "0.05", "--num_train_steps", "2000", "--freeze",
               "conv_blocks.0,conv_blocks.1", "--lr_scale", "conv_blocks=0.1", "--lr_scale", "event_fc=2", "--no_decay_norm_bias"])
    main.validate_args(a)
    model = sed.Cnn_AvgPooling(1, [(4, 2), (8, 2), (8, 2), (8, 1)], precision="fp32")
    opts = main.schedule_options(a, model)
    assert opts["lr_schedule"].as_dict() == dict(kind="cosine", warmup=500, total=2000, every=200, gamma=0.997, floor=0.05)
    pg = opts["param_groups"]
    assert pg[0] == {"params": ["conv_blocks.0", "conv_blocks.1"], "frozen": True}
    # the undecayed half of a prefix sits in front of the prefix: the first match wins
    assert pg[1]["lr_scale"] == 0.1 and pg[1]["weight_decay"] == 0.0 and all(n.startswith("conv_blocks.") for n in pg[1]["params"])
    assert pg[2] == {"params": ["conv_blocks"], "lr_scale": 0.1}
    assert pg[3] == {"params": ["event_fc.bias"], "lr_scale": 2.0, "weight_decay": 0.0}
    assert pg[4] == {"params": ["event_fc"], "lr_scale": 2.0} and len(pg) == 5
    names = [n for n, _ in model.named_parameters()]
    specs, asg = tr.resolve_param_groups(names, pg, 0.01)
    w = float(np.float32(0.01))
    for (n, q), g in zip(model.named_parameters(), asg):
        scale, wd, fz = specs[g]
        assert fz == n.startswith(("conv_blocks.0.", "conv_blocks.1.")), n
        if not fz:
            assert scale == (2.0 if n.startswith("event_fc") else float(np.float32(0.1))) and wd == (0.0 if q.ndim <= 1 else w), n
    vec = main.schedule_options(parse(["--no_decay_norm_bias", "--lr_scale", "event_fc.bias=3"]), model)["param_groups"]
    assert vec[0] == {"params": ["event_fc.bias"], "lr_scale": 3.0, "weight_decay": 0.0} and len(vec) == 2 and "lr_scale" not in vec[1]
    tr.resolve_param_groups(names, vec, 0.01)
    only = main.schedule_options(parse(["--no_decay_norm_bias"]), model)["param_groups"]
    assert len(only) == 1 and only[0]["weight_decay"] == 0.0 and set(only[0]["params"]) == {n for n, q in model.named_parameters() if q.ndim <= 1}
    assert main.schedule_options(parse(["--lr_schedule", "constant"]))["lr_schedule"].kind == "const"
    assert main.schedule_options(parse(["--lr_schedule", "linear", "--lr_total_steps", "77"]))["lr_schedule"].total == 77
    for bad in (["--warmup_steps", "5"], ["--lr_schedule", "cosine", "--warmup_steps", "-1"], ["--lr_schedule", "cosine", "--lr_floor", "2"],
                ["--lr_schedule", "linear", "--warmup_steps", "10", "--lr_total_steps", "10"], ["--lr_scale", "event_fc"],
                ["--lr_scale", "=0.5"], ["--lr_scale", "event_fc=abc"], ["--lr_scale", "event_fc=-1"], ["--freeze", ","]):
        with pytest.raises(ValueError):
            main.validate_args(parse(bad))
    with pytest.raises(SystemExit):
        parse(["--lr_schedule", "exponential"])
    # build_parser() keeps exactly the reference's flags plus the optimizer options
    assert not {"lr_schedule", "freeze", "lr_scale"} & set(vars(main.build_parser().parse_args([])))
    import inspect
    for fn in (tr.train, tr.FusedTrainer.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["lr_schedule"].default is None and sig["param_groups"].default is None
    assert "lr_schedule" not in inspect.signature(tr.FusedAdamAmsgrad.__init__).parameters


# ---- state_dict layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_state_dict_layout_loads_into_torch(tr, decoupled):
    names = [f"p{i}" for i in range(len(SHAPES))]
    specs = [(1.0, 1e-2, False), (0.1, 0.0, False), (2.5, 3e-2, False), (1.0, 1e-2, True)]
    template = {"lr": 0.0, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": True, "maximize": False, "foreach": None,
                "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": decoupled, "params": []}
    sched = tr.LRSchedule("cosine", warmup=3, total=8)
    base, step = 1e-3, 4
    pgs = tr.grouped_param_groups(template, specs, GROUP_OF_PARAM, tr.lr_at(base, step + 1, sched), base)
    assert [g["params"] for g in pgs] == [[0, 5], [1, 4], [2, 7], [3, 6]]
    assert [g["lr"] for g in pgs] == [tr.lr_at(base, 5, sched) * s for s, _, _ in specs]
    assert [g["initial_lr"] for g in pgs] == [base * s for s, _, _ in specs]
    assert [g["weight_decay"] for g in pgs] == [1e-2, 0, 3e-2, 1e-2] and [g["frozen"] for g in pgs] == [False, False, False, True]
    state = {i: {"step": torch.tensor(float(step)), "exp_avg": torch.full(s, 0.5), "exp_avg_sq": torch.full(s, 0.25),
                 "max_exp_avg_sq": torch.full(s, 0.3)} for i, s in enumerate(SHAPES) if not specs[GROUP_OF_PARAM[i]][2]}
    sd = {"state": state, "param_groups": pgs, "lr_schedule": dict(sched.as_dict(), base_lr=base)}
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    tgroups = [{"params": [params[i] for i in g["params"]], "weight_decay": g["weight_decay"]} for g in pgs]
    topt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(tgroups, lr=123.0, amsgrad=True)
    topt.load_state_dict(sd)
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in pgs]
    assert params[3] not in topt.state and params[6] not in topt.state, "no state for frozen parameters"
    assert float(topt.state[params[0]]["exp_avg"][0]) == 0.5 and int(topt.state[params[7]]["step"]) == step
    back = topt.state_dict()             # torch renumbers: ids follow the groups, one after the other
    assert [g["params"] for g in back["param_groups"]] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    assert tr.state_index_map(back["param_groups"], pgs) == {0: 0, 1: 5, 2: 1, 3: 4, 4: 2, 5: 7, 6: 3, 7: 6}
    assert tr.state_index_map(pgs, pgs) == {i: i for i in range(8)}
    for other in (pgs[:3], [dict(pgs[0], params=[0]), *pgs[1:]], [dict(pgs[0], params=[0, 5, 1]), dict(pgs[1], params=[4]), *pgs[2:]]):
        with pytest.raises(ValueError, match="parameter groups"):
            tr.state_index_map(other, pgs)
    # an empty remainder (every parameter matched) leaves no empty group behind
    assert [g["params"] for g in tr.grouped_param_groups({}, [(1.0, 0.0, False), (1.0, 0.0, False)], [1, 1], 0.0, 0.0)] == [[0, 1]]


def test_abi_refusals_without_gpu():
    """host-side checks fire before any launch (the pointers below are never dereferenced)"""
    L = importlib.import_module(PKG + "._lib")
    lib = L.lib()
    q = 4096

    def call(**kw):
        a = dict(p=q, g=q, m=q, v=q, vmax=q, n=64, tiles=q, nt=1, groups=q, ng=1, gh=q, hyper=q, step=q, base_lr=1e-3, kind=0, warmup=0,
                 total=0, every=200, gamma=0.997, floor=0.0)
        a.update(kw)
        return lib.sed_adam_groups_step(a["p"], a["g"], a["m"], a["v"], a["vmax"], a["n"], a["tiles"], a["nt"], a["groups"], a["ng"],
                                        a["gh"], a["hyper"], a["step"], a["base_lr"], a["kind"], a["warmup"], a["total"], a["every"],
                                        a["gamma"], a["floor"], 0.9, 0.999, 1e-8, 1.0, 0, None, None)

    bad = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(tiles=None), dict(groups=None), dict(gh=None), dict(hyper=None),
           dict(step=None), dict(p=q + 4), dict(vmax=q + 8), dict(tiles=q + 4), dict(nt=0), dict(ng=0), dict(ng=65), dict(kind=5),
           dict(kind=-1), dict(warmup=-1), dict(kind=2, warmup=5, total=5), dict(kind=3, total=0), dict(kind=1, every=0),
           dict(floor=-0.5), dict(floor=1.5), dict(floor=float("nan")), dict(gamma=0.0), dict(gamma=float("nan")),
           dict(base_lr=float("inf")), dict(base_lr=float("nan")), dict(n=0), dict(n=6)]
    for kw in bad:
        assert call(**kw) == 1 and b"sed_adam_groups_step" in lib.sed_last_error(), kw
    for args in ((None, 64, q, 1, q, 1.0, 1.0, q, q, None), (q, 64, None, 1, q, 1.0, 1.0, q, q, None), (q, 64, q, 1, None, 1.0, 1.0, q, q, None),
                 (q, 64, q, 1, q, 1.0, 1.0, None, q, None), (q, 64, q, 1, q, 1.0, 1.0, q, None, None), (q, 64, q, 0, q, 1.0, 1.0, q, q, None),
                 (q + 4, 64, q, 1, q, 1.0, 1.0, q, q, None), (q, 64, q, 1, q, 1.0, 1.0, q + 4, q, None), (q, 62, q, 1, q, 1.0, 1.0, q, q, None)):
        assert lib.sed_grad_norm_groups(*args) == 1 and b"sed_grad_norm_groups" in lib.sed_last_error(), args
