"""Gradient-norm clipping, host side: the three Lightning arguments of the trainer (gradient_clip_val, gradient_clip_algorithm, track_grad_norm), their
command-line flags, and the launch sequence the optimizers issue for them — with everything off, exactly the calls made before the feature existed."""
import importlib
import json
import os

import pytest
import torch


def test_trainer_validates_the_gradient_clipping_arguments():
    from enhancing.engine.trainer import Trainer
    tr = Trainer()
    assert tr.gradient_clip_val is None and tr.gradient_clip_algorithm == "norm" and tr.track_grad_norm == -1
    tr = Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value", track_grad_norm=2)
    assert tr.gradient_clip_val == 0.5 and tr.gradient_clip_algorithm == "value" and tr.track_grad_norm == 2
    assert Trainer(gradient_clip_val=0.0).gradient_clip_val is None          # Lightning: 0 = no clipping
    for bad in (dict(gradient_clip_val=-1.0), dict(gradient_clip_val=float("nan")), dict(gradient_clip_algorithm="global"), dict(track_grad_norm=1),
                dict(track_grad_norm=float("inf")), dict(track_grad_norm=0)):
        with pytest.raises(ValueError):
            Trainer(**bad)


def test_main_parser_accepts_the_three_flags():
    main = importlib.import_module("main")
    a = main.build_parser().parse_args(["-c", "x", "--gradient_clip_val", "1.5", "--gradient_clip_algorithm", "value", "--track_grad_norm", "2"])
    assert a.gradient_clip_val == 1.5 and a.gradient_clip_algorithm == "value" and a.track_grad_norm == 2
    d = main.build_parser().parse_args(["-c", "x"])
    assert d.gradient_clip_val is None and d.gradient_clip_algorithm == "norm" and d.track_grad_norm == -1
    for bad in (["--gradient_clip_algorithm", "global"], ["--track_grad_norm", "1"]):
        with pytest.raises(SystemExit):
            main.build_parser().parse_args(["-c", "x"] + bad)


class _Calls(list):
    today = new = None


class _Store:
    def __init__(self, n=256):
        self.p, self.g, self.m, self.v, self.step_count = torch.zeros(n), torch.ones(n), torch.zeros(n), torch.zeros(n), 0


@pytest.fixture
def calls(monkeypatch):
    """stand-ins for the four launches of a step, recording (name, positional count, keywords)"""
    from enhancing import _C
    rec = _Calls()

    def adamw_today(p, g, m, v, p16, step, lr, b1, b2, eps, wd, grad_scale, skip_flag=None, loss_scale=None):      # the signature before the feature
        rec.append(("adamw_step", grad_scale, dict(skip_flag=skip_flag, loss_scale=loss_scale)))

    def adamw_new(p, g, m, v, p16, step, lr, b1, b2, eps, wd, grad_scale, **kw):
        rec.append(("adamw_step", grad_scale, kw))
    monkeypatch.setattr(_C, "nonfinite_flag", lambda x, flag: rec.append(("nonfinite_flag",)))
    monkeypatch.setattr(_C, "loss_scale_update", lambda *a: rec.append(("loss_scale_update",)))
    monkeypatch.setattr(_C, "grad_clip_coef", lambda g, max_norm, grad_scale, out, loss_scale=None, found_inf=None:
                        rec.append(("grad_clip_coef", max_norm, grad_scale, loss_scale is not None, found_inf is not None)), raising=False)
    rec.today, rec.new = adamw_today, adamw_new
    return rec


def test_flat_adamw_launch_sequence(monkeypatch, calls):
    from enhancing import _C
    from enhancing.engine.optim import FlatAdamW, LossScaler
    st = _Store()
    opt = FlatAdamW(st, lr=1e-3)
    opt.grad_scale = 0.5
    # everything off: one AdamW launch with the positional signature of before, no keywords
    monkeypatch.setattr(_C, "adamw_step", calls.today)
    opt.step()
    assert calls == [("adamw_step", 0.5, dict(skip_flag=None, loss_scale=None))] and opt.grad_norm is None
    st.loss_scaler = LossScaler(torch.device("cpu"))
    st.loss_scaler.enabled = True
    del calls[:]
    opt.step()
    assert [c[0] for c in calls] == ["nonfinite_flag", "adamw_step", "loss_scale_update"]
    # clipping by norm under the scaler: the norm kernel REPLACES the flag pass and is handed the loss scale and the flag
    monkeypatch.setattr(_C, "adamw_step", calls.new)
    opt.gradient_clip_val = 2.0
    del calls[:]
    opt.step()
    assert [c[0] for c in calls] == ["grad_clip_coef", "adamw_step", "loss_scale_update"] and calls[0] == ("grad_clip_coef", 2.0, 0.5, True, True)
    kw = calls[1][2]
    assert kw["clip_coef"].data_ptr() == opt.grad_norm.data_ptr() + 4 and "clip_value" not in kw and kw["skip_flag"] is st.loss_scaler.found_inf
    # monitor only: the norm is measured, AdamW gets no coefficient
    opt.gradient_clip_val, opt.track_grad_norm = None, True
    st.loss_scaler.enabled = False
    del calls[:]
    opt.step()
    assert calls == [("grad_clip_coef", float("inf"), 0.5, False, False), ("adamw_step", 0.5, {})]
    # by value: no norm pass unless tracked
    opt.gradient_clip_val, opt.gradient_clip_algorithm, opt.track_grad_norm = 0.25, "value", False
    del calls[:]
    opt.step()
    assert calls == [("adamw_step", 0.5, dict(clip_value=0.25))]
    opt.gradient_clip_algorithm = "global"
    with pytest.raises(ValueError):
        opt.step()


_INF = float("inf")
# The launch table of the shared step (engine/optim.py scaled_step), written down from the three optimizers' steps as they were before they shared it.
# scaler: None | "disabled" | "on" | "nocheck" (the engine's ENH_NONFINITE_CHECK=0); clip = (clip_norm, clip_value); then the launches in order and
# the exact keyword set of the Adam launch.  The flag pass and the norm pass under a scaler that checks must find the flag zeroed.
_STEP_ROWS = [
    # id                 scaler      clip           unscaled  launches                                                  Adam keywords
    ("plain",            None,       (None, None),  False,    ["adam"],                                                 set()),
    ("disabled",         "disabled", (None, None),  False,    ["adam"],                                                 set()),
    ("norm",             None,       (2.0, None),   False,    ["grad_clip_coef", "adam"],                               {"clip_coef"}),
    ("disabled-norm",    "disabled", (2.0, None),   False,    ["grad_clip_coef", "adam"],                               {"clip_coef"}),
    ("track",            None,       (_INF, None),  False,    ["grad_clip_coef", "adam"],                               set()),
    ("value",            None,       (None, 0.25),  False,    ["adam"],                                                 {"clip_value"}),
    ("value-0",          None,       (None, 0),     False,    ["adam"],                                                 set()),
    ("scaled",           "on",       (None, None),  False,    ["nonfinite_flag", "adam", "loss_scale_update"],          {"skip_flag", "loss_scale"}),
    ("scaled-norm",      "on",       (2.0, None),   False,    ["grad_clip_coef", "adam", "loss_scale_update"],          {"skip_flag", "loss_scale", "clip_coef"}),
    ("scaled-track",     "on",       (_INF, None),  False,    ["grad_clip_coef", "adam", "loss_scale_update"],          {"skip_flag", "loss_scale"}),
    ("scaled-value",     "on",       (None, 0.25),  False,    ["nonfinite_flag", "adam", "loss_scale_update"],          {"skip_flag", "loss_scale", "clip_value"}),
    ("unscaled",         "on",       (None, None),  True,     ["nonfinite_flag", "adam", "loss_scale_update"],          {"skip_flag"}),
    ("unscaled-norm",    "on",       (2.0, None),   True,     ["grad_clip_coef", "adam", "loss_scale_update"],          {"skip_flag", "clip_coef"}),
    ("nocheck",          "nocheck",  (None, None),  False,    ["adam"],                                                 {"loss_scale"}),
    ("nocheck-norm",     "nocheck",  (2.0, None),   False,    ["grad_clip_coef", "adam"],                               {"loss_scale", "clip_coef"}),
]


@pytest.mark.parametrize("scaler,clip,unscaled,launches,adam_kw", [r[1:] for r in _STEP_ROWS], ids=[r[0] for r in _STEP_ROWS])
def test_shared_step_issues_the_rows_of_the_launch_table(monkeypatch, scaler, clip, unscaled, launches, adam_kw):
    from enhancing import _C
    from enhancing.engine.optim import LossScaler, scaled_step
    cpu = torch.device("cpu")
    sc = None if scaler is None else LossScaler(cpu, init_scale=8.0, growth_interval=7, enabled=scaler != "disabled", check=scaler != "nocheck",
                                                count_skipped=True)
    on = scaler == "on"
    if scaler in ("on", "disabled"):
        sc.found_inf.fill_(1.0)      # left over from an earlier step: a scaler that checks has to clear it before the pass that sets it
    g, out, rec = torch.ones(64), torch.zeros(2), []

    def flag_pass(x, flag):
        rec.append(("nonfinite_flag", x, flag, float(flag)))
        flag.fill_(1.0)              # "an inf was found": the dropped-step counter below must see it

    def norm_pass(x, max_norm, grad_scale, o, **kw):
        rec.append(("grad_clip_coef", x, max_norm, grad_scale, o, kw, None if kw.get("found_inf") is None else float(kw["found_inf"])))

    monkeypatch.setattr(_C, "nonfinite_flag", flag_pass)
    monkeypatch.setattr(_C, "grad_clip_coef", norm_pass)
    monkeypatch.setattr(_C, "loss_scale_update", lambda *a: rec.append(("loss_scale_update",) + a))
    scaled_step(g, 0.5, clip, out, sc, lambda **kw: rec.append(("adam", kw)), **(dict(grads_unscaled=True) if unscaled else {}))
    assert [r[0] for r in rec] == launches
    by_name = {r[0]: r for r in rec}
    scale_operand = on and not unscaled or scaler == "nocheck"      # the table: loss_scale reaches both launches or neither
    if "nonfinite_flag" in by_name:
        _, x, flag, seen = by_name["nonfinite_flag"]
        assert x is g and flag is sc.found_inf and seen == 0.0
    if "grad_clip_coef" in by_name:
        _, x, max_norm, grad_scale, o, kw, seen = by_name["grad_clip_coef"]
        assert x is g and max_norm == clip[0] and grad_scale == 0.5 and o is out
        assert set(kw) == ({"found_inf"} if on else set()) | ({"loss_scale"} if scale_operand else set())
        assert kw.get("found_inf") is (sc.found_inf if on else None) and kw.get("loss_scale") is (sc.scale_t if scale_operand else None)
        assert seen == (0.0 if on else None)
    kw = by_name["adam"][1]
    assert set(kw) == adam_kw and all(v is not None for v in kw.values())
    if "skip_flag" in kw:
        assert kw["skip_flag"] is sc.found_inf
    if "loss_scale" in kw:
        assert kw["loss_scale"] is sc.scale_t
    if "clip_coef" in kw:
        assert kw["clip_coef"].data_ptr() == out.data_ptr() + 4 and kw["clip_coef"].numel() == 1
    if "clip_value" in kw:
        assert kw["clip_value"] == clip[1]
    if on:
        upd = by_name["loss_scale_update"]
        assert upd[1] is sc.scale_t and upd[2] is sc.found_inf and upd[3] is sc.tracker and upd[4:] == (2.0, 0.5, 7)
        assert float(sc.skipped_steps) == (1.0 if "nonfinite_flag" in by_name else 0.0)      # counts what the flag pass left, after the update read it
    elif scaler == "disabled":
        assert float(sc.found_inf) == 1.0 and float(sc.skipped_steps) == 0.0                  # a disabled scaler is not touched
    elif scaler == "nocheck":
        assert sc.found_inf is None and sc.skipped_steps is None


def test_loss_scaler_reads_each_default_from_its_own_variable(monkeypatch):
    from enhancing.engine.optim import LossScaler
    cpu = torch.device("cpu")
    for v in ("ENH_LOSS_SCALE", "ENH_LOSS_NET_SCALE", "ENH_LOSS_SCALE_INTERVAL"):
        monkeypatch.delenv(v, raising=False)
    net, eng = LossScaler(cpu), LossScaler(cpu, env="ENH_LOSS_SCALE", enabled=True)
    assert (net.scale_t.item(), net.growth_interval, net.enabled, net.value) == (4096.0, 2000, False, 1.0) and net.skipped_steps is None
    assert (eng.scale_t.item(), eng.growth_interval, eng.enabled, eng.value) == (65536.0, 2000, True, 65536.0)
    monkeypatch.setenv("ENH_LOSS_SCALE", "1024")
    monkeypatch.setenv("ENH_LOSS_NET_SCALE", "256")
    monkeypatch.setenv("ENH_LOSS_SCALE_INTERVAL", "5")
    assert LossScaler(cpu).scale_t.item() == 256.0 and LossScaler(cpu, env="ENH_LOSS_SCALE").scale_t.item() == 1024.0
    assert LossScaler(cpu).growth_interval == 5 and LossScaler(cpu, init_scale=2.0, growth_interval=3).scale_t.item() == 2.0


def test_fused_and_flat_adamw_save_the_same_keys():
    from enhancing.engine.optim import FlatAdamW, FusedAdamW
    st = _Store()
    st.step_count, eng = 3, type("E", (), {})()
    eng.store = st
    for opt in (FlatAdamW(st, lr=1e-3), FusedAdamW(eng, lr=1e-3)):
        sd = opt.state_dict()
        assert sorted(sd) == ["m", "param_groups", "step", "v"] and sd["step"] == 3 and sd["param_groups"] is opt.param_groups
        st.m.fill_(0.0)
        opt.load_state_dict(dict(sd, step=5, m=torch.full_like(st.m, 2.0)))
        assert st.step_count == 5 and float(st.m[0]) == 2.0
        st.step_count = 3


def test_trainer_hands_the_switches_to_every_optimizer_and_logs_the_norms(monkeypatch, tmp_path):
    from enhancing.engine import trainer as T

    class Opt:
        def __init__(self, norm):
            self.param_groups, self.grad_scale, self.grad_norm, self.steps = [dict(lr=1.0)], 1.0, torch.tensor([norm]), 0

        def step(self):
            self.steps += 1

        def state_dict(self):
            return {}

    opts = [Opt(3.0), Opt(0.5)]

    class Model:
        logged, global_step = {}, 0
        engine = type("E", (), {"store": None})()

        def configure_optimizers(self):
            return opts, []

        def training_step(self, batch, batch_idx, optimizer_idx, zero_grad=True):
            self.logged["train/total_loss"] = torch.tensor(0.5)

        def state_dict(self):
            return {}

    class Data:
        dataset_configs = {"train": 1}

        def setup(self, rank, world):
            pass

        def train_dataloader(self):
            return [{"image": torch.zeros(2, 3, 8, 8)} for _ in range(2)]

    monkeypatch.setattr(T, "init_process_group_from_env", lambda *a, **k: (0, 0, 1))
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    T.Trainer(max_epochs=1, default_root_dir=str(tmp_path / "on"), log_every_n_steps=1, gradient_clip_val=1.5, track_grad_norm=2).fit(Model(), Data())
    for o in opts:
        assert o.gradient_clip_val == 1.5 and o.gradient_clip_algorithm == "norm" and o.track_grad_norm is True and o.steps == 2
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path / "on"), "metrics.jsonl"))]
    assert len(rows) == 2 and rows[0]["train/grad_norm"] == 3.0 and rows[0]["train/grad_norm_disc"] == 0.5
    T.Trainer(max_epochs=1, default_root_dir=str(tmp_path / "off"), log_every_n_steps=1).fit(Model(), Data())
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path / "off"), "metrics.jsonl"))]
    assert all(o.gradient_clip_val is None and o.track_grad_norm is False for o in opts) and "train/grad_norm" not in rows[0]
