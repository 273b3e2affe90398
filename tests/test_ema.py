"""EMA weight averaging on the CPU: the decay rule, the float64 oracle and ``ModelEma`` against torch's
``AveragedModel``, decay 0, the flags, the single-device entry point with ``--eval`` / ``.ema.pt`` / ``--eval-only``,
evaluation without touching the live model, resume, and ``evaluate_netresdeep(params=...)``."""
import argparse
import copy
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
from distributeddataparallel_cifar10_amd.utils.ema import ModelEma, ema_decay_at, ema_reference

CPU = torch.device("cpu")
TOL = 1e-6  # relative L2 per tensor: fp32 rounding of a subtract, a multiply and an add against float64


def test_ema_decay_at_values():
    assert [ema_decay_at(k, 0.999) for k in (0, 1, 10**6)] == [0.999] * 3
    assert ema_decay_at(0, 0.999, warmup=True) == 1 / 10
    assert ema_decay_at(1, 0.999, warmup=True) == 2 / 11
    assert ema_decay_at(90, 0.9, warmup=True) == 0.9  # 91 / 100 > 0.9
    assert ema_decay_at(80, 0.9, warmup=True) == 81 / 90  # = 0.9 exactly in the rationals, min() of equal floats
    assert ema_decay_at(79, 0.9, warmup=True) == 80 / 89
    assert ema_decay_at(10**7, 0.9999, warmup=True) == 0.9999
    assert ema_decay_at(5, 0.0, warmup=True) == 0.0
    ks = np.arange(0, 2000)
    ds = np.array([ema_decay_at(int(k), 0.99, True) for k in ks])
    assert np.all(np.diff(ds) >= 0) and ds[-1] == 0.99


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan")])
def test_ema_decay_rejects_bad_decay(bad):
    with pytest.raises(ValueError):
        ema_decay_at(0, bad)
    with pytest.raises(ValueError):
        ModelEma(nn.Linear(2, 2), bad)


def test_ema_decay_rejects_bad_step():
    with pytest.raises(ValueError):
        ema_decay_at(-1, 0.5)
    with pytest.raises(ValueError):
        ema_decay_at(1.5, 0.5)


def test_ema_reference_is_float64_and_exact_at_zero():
    e, p = np.float32([1.0, 2.0, -3.0]), torch.tensor([0.5, 4.0, 1.0])
    out = ema_reference(e, p, 0.25)
    assert out.dtype == np.float64 and np.array_equal(out, [0.625, 3.5, 0.0])
    assert np.array_equal(ema_reference(e, p, 0.0), p.double().numpy())


def _sgd_steps(model, n, seed=7, on_step=None):
    g = torch.Generator().manual_seed(seed)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    loss_fn = nn.CrossEntropyLoss()
    model.train()
    for k in range(n):
        x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
        loss = loss_fn(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if on_step:
            on_step(k)


@pytest.mark.parametrize("wrap", ["module", "flat"])
def test_model_ema_and_reference_match_averaged_model(wrap):
    """Five SGD steps of a CPU NetResDeep: ``ModelEma`` and a chain of ``ema_reference`` updates against torch's
    ``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d), use_buffers=True)``, <= 1e-6 relative L2 per tensor."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatBucketDDP
    d = 0.9
    torch.manual_seed(3)
    model = NetResDeep()
    wrapped = FlatBucketDDP(model) if wrap == "flat" else model  # world size 1: no process group needed
    theirs = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d), use_buffers=True)
    # AveragedModel copies on its first update; ModelEma starts from the model it is given: give torch's the same start
    theirs.update_parameters(model)
    ours = ModelEma(wrapped, d)
    uniq = {n: t for n, t in list(model.named_parameters()) + list(model.named_buffers())}
    ref = {n: t.detach().double().numpy().copy() for n, t in uniq.items() if t.is_floating_point()}

    def on_step(k):
        assert ours.update(k) == d
        theirs.update_parameters(model)
        for n in ref:
            ref[n] = ema_reference(ref[n], uniq[n], d)

    _sgd_steps(wrapped, 5, on_step=on_step)
    want = dict(list(theirs.module.named_parameters()) + list(theirs.module.named_buffers()))
    got = ours.state_dict()
    assert list(got) == list(model.state_dict()) and len(got) == 66
    worst = 0.0
    for n, w in want.items():
        if not w.is_floating_point():
            # num_batches_tracked is copied (5 steps x 10 applications of the one ResBlock); torch's AveragedModel
            # runs its integer buffers through the averaging function, which is not what a checkpoint should hold
            assert int(got[n]) == int(uniq[n]) == 50, n
            continue
        w64 = w.detach().double().numpy()
        for what, g in (("ModelEma", got[n].double().numpy()), ("ema_reference", ref[n])):
            err = float(np.linalg.norm(g - w64) / np.linalg.norm(w64))
            worst = max(worst, err)
            assert err <= TOL, (n, what, err)
        assert not torch.equal(got[n], uniq[n].detach()), n  # it is an average, not the live tensor
    print(f"{wrap}: worst relative L2 {worst:.3e}")
    assert got["resblocks.0.conv.weight"].data_ptr() == got["resblocks.9.conv.weight"].data_ptr()


def test_decay_zero_gives_the_model_bitwise():
    torch.manual_seed(4)
    model = NetResDeep()
    ema = ModelEma(model, 0.0, warmup=True)
    sd = model.state_dict()

    def on_step(k):
        assert ema.update(k) == 0.0
        avg = ema.state_dict()
        for key in sd:
            assert torch.equal(avg[key], sd[key]), (k, key)

    _sgd_steps(model, 3, on_step=on_step)


def test_warmup_decays_are_applied_in_order():
    lin = nn.Linear(1, 1, bias=False)
    with torch.no_grad():
        lin.weight.fill_(0.0)
    ema = ModelEma(lin, 0.5, warmup=True)
    want = 0.0
    for k in range(6):
        with torch.no_grad():
            lin.weight.fill_(float(k + 1))
        d = ema.update(k)
        assert d == min(0.5, (1 + k) / (10 + k)) == ema.last_decay
        want = (k + 1) + d * (want - (k + 1))
        assert abs(float(ema.params["weight"]) - want) <= 1e-6 * abs(want)


# ---- flags -----------------------------------------------------------------------------------------------------
def _parse(argv, batch_default=32):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser(), batch_default).parse_args(argv), "data/CIFAR-10/")


def test_flags_parse_and_defaults_are_todays():
    from distributeddataparallel_cifar10_amd import train as T
    cfg = _parse([])
    assert cfg == T.TrainConfig(data_path="data/CIFAR-10/")
    assert cfg.ema_decay is None and cfg.ema_warmup is False
    assert not T.optimizer_active(cfg) and T.engine_optimizer(cfg, 10) is None
    on = _parse(["--ema-decay", "0.99"])
    assert on.ema_decay == 0.99 and on.ema_warmup is False and T.optimizer_active(on)
    opt = T.engine_optimizer(_parse(["--ema-decay", "0.99", "--ema-warmup", "--epochs", "2"]), 5)
    assert (opt.momentum, opt.weight_decay, opt.ema_decay, opt.ema_warmup) == (0.0, 0.0, 0.99, True)
    assert list(opt.lr_table) == [1e-2] * 10  # a constant table when no schedule is given
    plain = T.engine_optimizer(_parse(["--momentum", "0.9"]), 5)
    assert plain.ema_decay is None and plain.ema_warmup is False
    assert _parse(["--ema-decay", "0"]).ema_decay == 0.0
    for bad in ("1.0", "-0.5"):
        with pytest.raises(SystemExit):
            _parse(["--ema-decay", bad])


# ---- the entry point ---------------------------------------------------------------------------------------------
def _run_main_no_ddp(monkeypatch, argv, **over):
    import main_no_ddp as M
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    cfg = config_from_args(add_cli_args(argparse.ArgumentParser(), batch_default=64).parse_args(argv), M.data_path)
    cfg.checkpoint = False  # as the script sets it ...
    for k, v in over.items():
        setattr(cfg, k, v)  # ... unless the test asks for the checkpoint files
    monkeypatch.setattr(M, "_cfg", cfg)
    monkeypatch.setattr(M, "device", CPU)
    torch.manual_seed(11)
    model = NetResDeep()
    M.training_loop(model, M.prepare())
    return M, cfg, model


def test_main_no_ddp_cpu_with_ema(tmp_path, monkeypatch, capsys):
    """main_no_ddp.py --synthetic 256 --epochs 2 --ema-decay 0.9 --eval on the CPU (with the checkpoint the script
    itself never writes switched on, for the .ema.pt): the EMA line, the metrics fields, the 66-key file that loads
    strictly, and --eval-only --resume of that file giving the printed EMA accuracy of the checkpoint's epoch."""
    from distributeddataparallel_cifar10_amd.train import eval_only
    mj, ck = tmp_path / "metrics.json", str(tmp_path / "ck" / "birds_vs_airplanes.pt")
    argv = ["--synthetic", "256", "--epochs", "2", "--ema-decay", "0.9", "--eval", "64", "--metrics-json", str(mj)]
    M, cfg, model = _run_main_no_ddp(monkeypatch, argv, checkpoint=True, checkpoint_path=ck)
    out = capsys.readouterr().out
    lines = re.findall(r"Epoch (\d+), EMA test accuracy (\d\.\d{4}), EMA test loss (\S+)", out)
    assert [ln[0] for ln in lines] == ["1", "2"], out
    assert len(re.findall(r"Epoch \d+, Test accuracy", out)) == 2
    recs = [r for r in map(json.loads, mj.read_text().splitlines()) if "epoch" in r]
    assert len(recs) == 2
    for r, ln in zip(recs, lines):
        assert r["ema_decay"] == 0.9
        assert "{:.4f}".format(r["ema_eval_accuracy"]) == ln[1] and repr(r["ema_eval_loss"]) == ln[2]
        assert np.isfinite(r["ema_eval_loss"]) and r["ema_eval_loss"] != r["eval_loss"]
    assert sorted(os.listdir(tmp_path / "ck")) == [
        "birds_vs_airplanes.pt", "birds_vs_airplanes.pt.ema.pt", "birds_vs_airplanes.pt.meta.json",
        "birds_vs_airplanes.pt.optim.pt"]
    avg = torch.load(ck + ".ema.pt", weights_only=True)
    assert len(avg) == 66 and list(avg) == list(NetResDeep().state_dict())
    ref = NetResDeep()
    ref.load_state_dict(avg, strict=True)
    assert int(avg["resblocks.0.batch_norm.num_batches_tracked"]) == 4 * 10  # epoch 1: 4 steps x 10 applications
    assert not torch.equal(avg["fc1.weight"], torch.load(ck, weights_only=True)["fc1.weight"])
    # the file is the epoch-1 average (checkpoints are written at logged epochs: 1, 10, ...)
    again = copy.copy(cfg)
    again.eval_only, again.resume = True, ck + ".ema.pt"
    res = eval_only(again, CPU)
    out2 = capsys.readouterr().out
    assert "{:.4f}".format(res.accuracy) == lines[0][1] and repr(res.mean_loss) == lines[0][2], (out2, lines)


def test_without_the_flag_nothing_is_written_or_printed(tmp_path, monkeypatch, capsys):
    mj, ck = tmp_path / "metrics.json", str(tmp_path / "ck" / "birds_vs_airplanes.pt")
    argv = ["--synthetic", "128", "--epochs", "1", "--eval", "32", "--metrics-json", str(mj)]
    _run_main_no_ddp(monkeypatch, argv, checkpoint=True, checkpoint_path=ck)
    assert "EMA" not in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "ck")) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json"]
    rec = [r for r in map(json.loads, mj.read_text().splitlines()) if "epoch" in r][0]
    assert rec["ema_decay"] is None and "ema_eval_accuracy" not in rec and "ema_eval_loss" not in rec


@pytest.mark.parametrize("wrap", ["module", "flat"])
def test_ema_evaluation_restores_the_live_model_bitwise(wrap):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.parallel.flat_ddp import FlatBucketDDP
    from distributeddataparallel_cifar10_amd.train import TrainConfig, run_eval
    torch.manual_seed(5)
    model = NetResDeep()
    wrapped = FlatBucketDDP(model) if wrap == "flat" else model
    ema = ModelEma(wrapped, 0.5)
    _sgd_steps(wrapped, 3, on_step=ema.update)
    data, labels = synthetic_cifar(48, seed=2)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in model.state_dict().items()}
    flags = [m.training for m in model.modules()]
    live = run_eval(wrapped, data, labels, TrainConfig())
    avg = run_eval(wrapped, data, labels, TrainConfig(), ema=ema)
    after = model.state_dict()
    for k in before:
        assert torch.equal(after[k], before[k]) and after[k].data_ptr() == ptrs[k], k
    assert flags == [m.training for m in model.modules()]
    assert avg.count == live.count == 48 and avg.loss_sum != live.loss_sum
    twin = NetResDeep()
    twin.load_state_dict(ema.state_dict(), strict=True)
    want = run_eval(twin, data, labels, TrainConfig())
    assert avg.loss_sum == want.loss_sum and torch.equal(avg.pred, want.pred)


def _main_cpu_run(seed, **kw):
    """One run of main.py's per-rank flow (world size 1, CPU: FlatBucketDDP + FlatSGD) with EMA; returns the final
    state and the final average."""
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.utils.checkpoint import export_state_dict
    cfg = T.TrainConfig(synthetic=256, max_steps=4, engine="torch", momentum=0.9, ema_decay=0.9, ema_warmup=True, **kw)
    data, labels = T.load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=CPU,
                          sampler="distributed", seed=0)
    torch.manual_seed(seed)
    model = T.build_model_for_rank(cfg, 0, 1, CPU, data, labels, loader)
    made = []
    real = ModelEma.__init__

    def spy(self, *a, **k):
        real(self, *a, **k)
        made.append(self)

    ModelEma.__init__ = spy
    try:
        T.train_loop(model, loader, 0, cfg)
    finally:
        ModelEma.__init__ = real
    assert len(made) == 1
    return export_state_dict(model), {k: v.detach().clone() for k, v in made[0].state_dict().items()}


def test_resume_restores_the_average_cpu(tmp_path, capsys):
    """One epoch plus --resume equals two epochs straight, bitwise, average included; without the .ema.pt the resume
    warns on stderr and restarts the average from the loaded parameters."""
    a, b = str(tmp_path / "a" / "birds_vs_airplanes.pt"), str(tmp_path / "b" / "birds_vs_airplanes.pt")
    straight, avg_straight = _main_cpu_run(5, epochs=2, checkpoint_path=a)
    _main_cpu_run(5, epochs=1, checkpoint_path=b)
    assert os.path.exists(b + ".ema.pt") and len(torch.load(b + ".ema.pt", weights_only=True)) == 66
    capsys.readouterr()
    resumed, avg_resumed = _main_cpu_run(99, epochs=2, resume=b, checkpoint=False)
    assert "warning" not in capsys.readouterr().err
    for name in straight:
        assert torch.equal(resumed[name], straight[name]), name
        assert torch.equal(avg_resumed[name], avg_straight[name]), name
    os.remove(b + ".ema.pt")
    cold, avg_cold = _main_cpu_run(99, epochs=2, resume=b, checkpoint=False)
    assert "ema.pt" in capsys.readouterr().err
    assert torch.equal(cold["fc1.weight"], straight["fc1.weight"])  # the live model does not depend on the average
    assert not torch.equal(avg_cold["fc1.weight"], avg_straight["fc1.weight"])


def test_evaluate_netresdeep_params():
    """evaluate_netresdeep(params=...) equals evaluating a model loaded with those tensors; the model is untouched."""
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_netresdeep
    torch.manual_seed(8)
    model, other = NetResDeep(), NetResDeep()
    data, labels = synthetic_cifar(40, seed=4)
    params = {n: p.detach().clone() for n, p in other.named_parameters()}
    assert len(params) == 9
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    datas = [p.data for p in model.parameters()]
    got = evaluate_netresdeep(model, data, labels, params=params, return_logits=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.data is d or p.data.data_ptr() == d.data_ptr() for p, d in zip(model.parameters(), datas))
    twin = copy.deepcopy(model)  # the model's own running statistics, the other's parameters
    twin.load_state_dict({**model.state_dict(), **{k: v for k, v in other.state_dict().items()
                                                   if "running" not in k and "num_batches" not in k}})
    want = evaluate_netresdeep(twin, data, labels, return_logits=True)
    assert torch.equal(got.logits, want.logits) and got.loss_sum == want.loss_sum and torch.equal(got.pred, want.pred)
    plain = evaluate_netresdeep(model, data, labels, return_logits=True)
    assert not torch.equal(plain.logits, got.logits)
    with pytest.raises(ValueError):
        evaluate_netresdeep(model, data, labels, params={"fc1.weight": params["fc1.weight"]})
    bad = dict(params, **{"fc2.bias": torch.zeros(11)})
    with pytest.raises(ValueError):
        evaluate_netresdeep(model, data, labels, params=bad)
