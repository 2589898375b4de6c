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
