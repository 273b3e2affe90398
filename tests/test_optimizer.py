"""Momentum, weight decay and per-step learning-rate schedules on the CPU: the schedule tables against torch's
schedulers, the float64 oracle of the engine's optimiser pass against ``torch.optim.SGD``, the default flags (nothing
changes), the training loop fed by the table, and resume with momentum buffers."""
import argparse
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from distributeddataparallel_cifar10_amd.utils.schedule import lr_at, lr_table, sgd_reference

CPU = torch.device("cpu")


def _torch_schedule(kind, base_lr, total, warm, min_lr, step_size, gamma):
    """The learning rate torch uses at every step: SequentialLR([LambdaLR warm-up, main schedule], [warm])."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, SequentialLR, StepLR
    p = nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=base_lr)

    def main(o):
        if kind == "constant":
            return LambdaLR(o, lambda s: 1.0)
        if kind == "step":
            return StepLR(o, step_size=step_size, gamma=gamma)
        return CosineAnnealingLR(o, T_max=total - warm, eta_min=min_lr)

    if warm:
        sched = SequentialLR(opt, [LambdaLR(opt, lambda s: (s + 1) / (warm + 1)), main(opt)], milestones=[warm])
    else:
        sched = main(opt)
    out = []
    for _ in range(total):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return np.asarray(out, dtype=np.float64)


@pytest.mark.parametrize("kind,warm,min_lr,step_size,gamma", [
    ("constant", 0, 0.0, None, 0.1), ("constant", 5, 0.0, None, 0.1),
    ("step", 0, 0.0, 7, 0.1), ("step", 3, 0.0, 4, 0.5),
    ("cosine", 0, 0.0, None, 0.1), ("cosine", 4, 1e-4, None, 0.1), ("cosine", 1, 0.0, None, 0.1),
])
def test_lr_table_matches_torch_schedulers(kind, warm, min_lr, step_size, gamma):
    import warnings
    total, base = 29, 0.05
    got = lr_table(kind, base, total, warmup_steps=warm, min_lr=min_lr, step_size=step_size, gamma=gamma)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SequentialLR's own deprecation chatter
        want = _torch_schedule(kind, base, total, warm, min_lr, step_size, gamma)
    assert got.shape == (total,) and got.dtype == np.float64
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("max relative difference", rel.max())
    assert rel.max() <= 1e-12, (got, want)
    assert lr_at(got, total + 10) == got[-1] and lr_at(got, 0) == got[0]


def test_lr_table_rejects_bad_arguments():
    with pytest.raises(ValueError):
        lr_table("linear", 0.1, 10)
    with pytest.raises(ValueError):
        lr_table("step", 0.1, 10)
    with pytest.raises(ValueError):
        lr_table("cosine", 0.1, 0)


def test_sgd_reference_matches_torch_sgd():
    """Three steps on random tensors against torch.optim.SGD(momentum=0.9, weight_decay=5e-4) in fp32: fp32 rounding of
    the three fused operations per step gives <= 2.4e-7 relative L2; the bound is 1e-6."""
    g = torch.Generator().manual_seed(3)
    shapes = [(32, 2048), (10, 32), (32,), (32, 32, 3, 3)]
    params = [nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4)
    ref_p = [p.detach().double().numpy().copy() for p in params]
    ref_b = [np.zeros_like(x) for x in ref_p]
    for k, lr in enumerate((0.1, 0.05, 0.2)):
        grads = [torch.randn(s, generator=g) for s in shapes]
        for grp in opt.param_groups:
            grp["lr"] = lr
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        for i, gr in enumerate(grads):
            ref_p[i], ref_b[i] = sgd_reference(ref_p[i], gr, ref_b[i], lr, 0.9, 5e-4)
            for name, got, want in (("param", params[i].detach(), ref_p[i]),
                                    ("buffer", opt.state[params[i]]["momentum_buffer"], ref_b[i])):
                err = np.linalg.norm(got.double().numpy() - want) / np.linalg.norm(want)
                print(f"step {k} tensor {i} {name}: relative L2 {err:.3e}")
                assert err <= 1e-6, (k, i, name, err)
    # inv_ws averages the summed gradient
    p1, b1 = sgd_reference(np.ones(4), 2 * np.ones(4), np.zeros(4), 0.5, 0.0, 0.0, inv_ws=0.5)
    assert np.array_equal(b1, np.ones(4)) and np.array_equal(p1, 0.5 * np.ones(4))


# ---- defaults: nothing changes ----------------------------------------------------------------------------------
def _parse(argv):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser()).parse_args(argv), "data/CIFAR-10/")


def test_default_flags_give_todays_config_and_optimizers(monkeypatch):
    from distributeddataparallel_cifar10_amd import train as T
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel import flat_ddp
    cfg = _parse([])
    assert cfg == T.TrainConfig(data_path="data/CIFAR-10/")
    assert (cfg.momentum, cfg.weight_decay, cfg.lr_schedule, cfg.lr_warmup_steps) == (0.0, 0.0, None, 0)
    assert not T.optimizer_active(cfg) and T.lr_table_for(cfg, 10) is None and T.engine_optimizer(cfg, 10) is None
    for argv in (["--momentum", "0.9"], ["--weight-decay", "1e-4"], ["--lr-schedule", "constant"],
                 ["--lr-warmup-steps", "3"]):
        assert T.optimizer_active(_parse(argv)), argv
    on = T.engine_optimizer(_parse(["--momentum", "0.9", "--lr-schedule", "cosine", "--epochs", "2"]), 5)
    assert on.momentum == 0.9 and on.weight_decay == 0.0 and len(on.lr_table) == 10

    made = []

    class SpySGD(torch.optim.SGD):
        def __init__(self, params, **kw):
            made.append(("torch", kw))
            super().__init__(params, **kw)

    class SpyFlat(flat_ddp.FlatSGD):
        def __init__(self, ddp, *a, **kw):
            made.append(("flat", a, kw))
            super().__init__(ddp, *a, **kw)

    monkeypatch.setattr(torch.optim, "SGD", SpySGD)
    monkeypatch.setattr(flat_ddp, "FlatSGD", SpyFlat)
    data, labels = synthetic_cifar(32, seed=0)
    loader = DeviceLoader(data, labels, batch_size=32, world_size=1, rank=0, device="cpu")
    run = T.TrainConfig(epochs=1, max_steps=1, checkpoint=False, lr=0.02)
    T.train_loop(NetResDeep(), loader, 0, run)
    T.train_loop(flat_ddp.FlatBucketDDP(NetResDeep()), loader, 0, run)
    assert made == [("torch", {"lr": 0.02}), ("flat", (0.02,), {})], made


# ---- the training loop fed by the table ---------------------------------------------------------------------------
def test_main_no_ddp_cpu_matches_hand_written_loop(tmp_path, monkeypatch, capsys):
    """main_no_ddp.py --synthetic 256 --epochs 2 --momentum 0.9 --weight-decay 5e-4 --lr-schedule cosine
    --lr-warmup-steps 2 on the CPU: the metrics' lr values are the table's, the final state_dict is bitwise that of a
    hand-written loop with torch.optim.SGD fed the same table."""
    import main_no_ddp as M
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args, load_dataset
    mj = tmp_path / "metrics.json"
    argv = ["--synthetic", "256", "--epochs", "2", "--momentum", "0.9", "--weight-decay", "5e-4", "--lr-schedule",
            "cosine", "--lr-warmup-steps", "2", "--metrics-json", str(mj)]
    cfg = config_from_args(add_cli_args(argparse.ArgumentParser(), batch_default=64).parse_args(argv), M.data_path)
    cfg.checkpoint = False
    monkeypatch.setattr(M, "_cfg", cfg)
    monkeypatch.setattr(M, "device", CPU)
    torch.manual_seed(11)
    model = NetResDeep()
    twin = copy.deepcopy(model)
    M.training_loop(model, M.prepare())

    table = lr_table("cosine", 1e-2, 8, warmup_steps=2)  # 256 images / batch 64 = 4 steps per epoch, 2 epochs
    recs = [json.loads(ln) for ln in mj.read_text().splitlines()]
    lrs = [r["lr"] for r in recs if "epoch" in r]
    assert lrs == [table[3], table[7]], (lrs, table)

    data, labels = load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=64, device=CPU, sampler="random", seed=cfg.seed)
    opt = torch.optim.SGD(twin.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    loss_fn, k = nn.CrossEntropyLoss(), 0
    for epoch in (1, 2):
        loader.set_epoch(epoch)
        for imgs, lab in loader:
            for grp in opt.param_groups:
                grp["lr"] = float(table[k])
            loss = loss_fn(twin(imgs), lab)
            opt.zero_grad()
            loss.backward()
            opt.step()
            k += 1
    assert k == 8
    sd, want = model.state_dict(), twin.state_dict()
    assert list(sd) == list(want)
    for name in sd:
        assert torch.equal(sd[name], want[name]), name


def _main_cpu_run(seed, **kw):
    """One run of main.py's per-rank flow (world size 1, CPU: FlatBucketDDP + FlatSGD); returns the final state."""
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import export_state_dict
    cfg = TrainConfig(synthetic=256, max_steps=4, engine="torch", momentum=0.9, weight_decay=5e-4, **kw)
    data, labels = load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=CPU,
                          sampler="distributed", seed=0)
    torch.manual_seed(seed)
    model = build_model_for_rank(cfg, 0, 1, CPU, data, labels, loader)
    train_loop(model, loader, 0, cfg)
    return export_state_dict(model)


def test_resume_restores_momentum_cpu(tmp_path):
    """Two epochs straight against one epoch + --resume, with momentum: bitwise equal final state.  The 66-key
    checkpoint is unchanged; the momentum buffers travel in <checkpoint>.optim.pt and the schedule position in the
    .meta.json sidecar.  Without the .optim.pt restore the states differ."""
    a, b = str(tmp_path / "a" / "birds_vs_airplanes.pt"), str(tmp_path / "b" / "birds_vs_airplanes.pt")
    straight = _main_cpu_run(5, epochs=2, checkpoint_path=a)
    _main_cpu_run(5, epochs=1, checkpoint_path=b)
    assert sorted(os.listdir(tmp_path / "b")) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                                  "birds_vs_airplanes.pt.optim.pt"]
    assert len(torch.load(b, weights_only=True)) == 66
    meta = json.load(open(b + ".meta.json"))
    assert meta == {"epoch": 1, "step": 4, "opt_step": 4}
    side = torch.load(b + ".optim.pt", weights_only=True)
    assert side["step"] == 4 and len(side["momentum_buffer"]) == 9
    assert all(float(v.abs().sum()) > 0 for v in side["momentum_buffer"].values())
    resumed = _main_cpu_run(99, epochs=2, resume=b, checkpoint=False)  # (another init seed: the checkpoint decides)
    assert list(resumed) == list(straight)
    for name in straight:
        assert torch.equal(resumed[name], straight[name]), name
    os.remove(b + ".optim.pt")  # the same resume without the momentum buffers: they restart at zero
    cold = _main_cpu_run(99, epochs=2, resume=b, checkpoint=False)
    assert not torch.equal(cold["fc1.weight"], straight["fc1.weight"])
