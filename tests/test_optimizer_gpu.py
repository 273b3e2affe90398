"""The fused engine's optimiser pass (csrc/optimizer.hip: momentum, weight decay, per-step learning-rate table) on an
MI355X: every update against the float64 oracle ``utils/schedule.sgd_reference``, the derived weight copies, graph
replay, the default (mu = wd = 0) identity with the fused SGD, two ranks on one GPU, and the entry point with resume.

All cases: 256 synthetic images, batch 8 unless stated (the pass's size is the fixed 76,140-float buffer).  Tolerance of
an update: <= 1e-6 relative L2 per tensor (three fp32 fused multiply-adds against float64: <= 2.4e-7)."""
import copy
import functools
import json
import os
import re
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist

from _ranks import spawn_ranks
from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MU, WD, TABLE = 0.9, 5e-4, [0.01, 0.02, 0.03, 0.015]
NDATA, B = 256, 8
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}
TOL = 1e-6


def _engine(dtype, persistent, optimizer, batch_max=B, seed=11, **kw):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    dev = torch.device("cuda", 0)
    data, labels = synthetic_cifar(NDATA, seed=3)
    torch.manual_seed(seed)
    model = NetResDeep().to(dev)
    eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                           EngineConfig(batch_max=batch_max, dtype=dtype, persistent=persistent, optimizer=optimizer,
                                        **kw))
    eng.set_indices(list(range(NDATA)))
    eng.set_cursor(0)
    eng.read_loss(reset=True)
    return model, eng


def _opt():
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    return OptimizerConfig(momentum=MU, weight_decay=WD, lr_table=TABLE)


def _snap(eng):
    eng.sync()
    return dict(params=eng.flat.detach().cpu().clone(), grads=eng.grads.detach().cpu().clone(),
                buf=eng.momentum.detach().cpu().clone(), step=eng.optimizer_step(), loss=eng.read_loss()[0])


@functools.lru_cache(maxsize=None)
def _eager_steps(kind):
    """Five single eager steps with momentum, weight decay and the table; the state before and after every step."""
    dtype, persistent = ENGINES[kind]
    model, eng = _engine(dtype, persistent, _opt())
    assert eng.kind_name == ("sliced" if persistent else "multikernel")
    snaps = [_snap(eng)]
    for _ in range(5):
        eng.run(B, 1, graph=False)
        snaps.append(_snap(eng))
    eng.check_errors()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    eng.close()
    return snaps, state


def _check_update(prev, cur, lr, inv_ws=1.0, tag=""):
    """cur's params and buffer = sgd_reference(prev params, cur grads, prev buffer, lr), per tensor."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.schedule import sgd_reference
    worst = 0.0
    for name, (off, shape) in LAYOUT.items():
        sl = slice(off, off + int(np.prod(shape)))
        want_p, want_b = sgd_reference(prev["params"][sl], cur["grads"][sl], prev["buf"][sl], lr, MU, WD, inv_ws)
        for what, got, want in (("param", cur["params"][sl], want_p), ("buffer", cur["buf"][sl], want_b)):
            err = float(np.linalg.norm(got.double().numpy() - want) / max(np.linalg.norm(want), 1e-300))
            worst = max(worst, err)
            assert err <= TOL, (tag, name, what, err)
        assert float(cur["grads"][sl].abs().sum()) > 0, (tag, name, "no gradient")
    print(f"{tag}: worst relative L2 {worst:.3e}")


@pytest.mark.parametrize("kind", list(ENGINES))
def test_per_step_update_matches_reference(gpu, kind):
    snaps, _ = _eager_steps(kind)
    assert snaps[0]["step"] == 0 and float(snaps[0]["buf"].abs().sum()) == 0.0
    for k in range(5):
        lr = TABLE[min(k, len(TABLE) - 1)]  # the fifth step holds the last table entry
        _check_update(snaps[k], snaps[k + 1], lr, tag=f"{kind} step {k}")
        assert snaps[k + 1]["step"] == k + 1
        assert np.isfinite(snaps[k + 1]["loss"])


@pytest.mark.parametrize("kind", list(ENGINES))
def test_derived_copies_follow_the_update(gpu, kind):
    """A twin that re-derives every kernel-layout weight copy from the fp32 parameters after each step: bitwise the
    same parameters and losses after four steps -- a layout copy the pass missed would diverge here."""
    snaps, _ = _eager_steps(kind)
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt())
    for _ in range(4):
        eng.run(B, 1, graph=False)
        eng.derive()
    twin = _snap(eng)
    eng.close()
    assert torch.equal(twin["params"], snaps[4]["params"]) and torch.equal(twin["buf"], snaps[4]["buf"])
    assert twin["loss"] == snaps[4]["loss"], (twin["loss"], snaps[4]["loss"])


@pytest.mark.parametrize("kind", list(ENGINES))
def test_graph_replay_equals_eager_steps(gpu, kind):
    """One 4-step graph replay (the table, the step counter and the hyper-parameters are read from device memory inside
    the captured graph) is bitwise the four eager steps; a second replay after set_lr_table picks the new table up
    without re-capture."""
    snaps, _ = _eager_steps(kind)
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt())
    eng.run(B, 4, graph=True)
    got = _snap(eng)
    assert got["step"] == 4
    assert torch.equal(got["params"], snaps[4]["params"]) and torch.equal(got["buf"], snaps[4]["buf"])
    assert got["loss"] == snaps[4]["loss"], (got["loss"], snaps[4]["loss"])
    eng.set_lr_table([0.0] * 8)  # learning rate 0 from the same captured graph: parameters stay, the buffer moves
    eng.run(B, 4, graph=True)
    after = _snap(eng)
    eng.close()
    assert after["step"] == 8 and torch.equal(after["params"], got["params"])
    assert not torch.equal(after["buf"], got["buf"])


def _five_steps(dtype, persistent, optimizer, batch=32):
    model, eng = _engine(dtype, persistent, optimizer, batch_max=batch)
    eng.run(batch, 5)
    loss, steps = eng.read_loss()
    assert steps == 5
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    eng.close()
    return loss, state


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_default_optimizer_is_the_fused_sgd_sliced(gpu, dtype):
    """OptimizerConfig() (mu = wd = 0, constant lr) on the sliced engine, batch 32, 5 steps: bitwise the state and loss
    of optimizer=None -- fmaf(0, p, g) = g, fmaf(0, buf, g) = g, fmaf(-lr, g, p) is the fused step's update."""
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    l0, s0 = _five_steps(dtype, True, None)
    l1, s1 = _five_steps(dtype, True, OptimizerConfig())
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_default_optimizer_multikernel(gpu):
    """The multi-kernel engine's fused SGD rounds p - lr * g in two operations, the pass in one fused multiply-add: the
    bounds of test_rccl_path_world_size_one (loss 1e-4 relative, tensors 2e-3 relative L2)."""
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    l0, s0 = _five_steps("fp32", False, None)
    l1, s1 = _five_steps("fp32", False, OptimizerConfig())
    assert abs(l0 - l1) <= 1e-4 * abs(l0), (l0, l1)
    for k in s0:
        a, b = s0[k].double(), s1[k].double()
        err = ((a - b).norm() / max(b.norm().item(), 1e-30)).item()
        assert err <= 2e-3, (k, err)


def test_optimizer_state_round_trip(gpu):
    """optimizer_state() views the flat buffer through LAYOUT; load_optimizer_state restores buffers and step."""
    snaps, _ = _eager_steps("sliced-bf16")
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    _, eng = _engine("bf16", True, _opt())
    with pytest.raises(ValueError):
        eng.load_optimizer_state({"step": 1, "momentum_buffer": {}})
    state = {"step": 3, "momentum_buffer": {
        name: snaps[3]["buf"][off:off + int(np.prod(shape))].view(shape) for name, (off, shape) in LAYOUT.items()}}
    eng.load_optimizer_state(state)
    got = eng.optimizer_state()
    assert got["step"] == 3 and set(got["momentum_buffer"]) == set(LAYOUT)
    for name, (off, shape) in LAYOUT.items():
        assert tuple(got["momentum_buffer"][name].shape) == shape
        assert torch.equal(got["momentum_buffer"][name].cpu(), state["momentum_buffer"][name])
    _, plain = _engine("bf16", True, None)
    with pytest.raises(RuntimeError, match="no optimiser"):
        plain.set_lr_table([0.1])
    plain.close()
    eng.close()


# ---- two ranks sharing one GPU --------------------------------------------------------------------------------
def _rank_worker(rank, ws, port, dtype, persistent, comm, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["DCA_XGMI_TIMEOUT_S"] = "30"  # a protocol bug ends as an error flag, not a hang
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        from distributeddataparallel_cifar10_amd.data.sampler import distributed_indices
        from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.ddp import FusedDDPTrainer, broadcast_module_state
        from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        data, labels = synthetic_cifar(NDATA, seed=5)
        order = distributed_indices(NDATA, ws, rank)
        torch.manual_seed(100 + rank)
        model = NetResDeep()
        broadcast_module_state(model, 0)
        model = model.to(dev)
        tr = None
        if comm == "xgmi":
            tr = FusedDDPTrainer(model, data.to(dev), labels.to(dev), batch_max=B, dtype=dtype, persistent=persistent,
                                 comm="xgmi", max_indices=len(order), optimizer=_opt())
            assert tr.comm == "xgmi", tr.comm
            eng = tr.engine
        else:
            eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                                   EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, world_size=ws,
                                                rank=rank, comm="external", optimizer=_opt()))
        eng.set_indices(order)
        eng.set_cursor(0)
        eng.read_loss(reset=True)

        def allreduce(t):
            h = t.cpu()
            dist.all_reduce(h)
            t.copy_(h.to(t.device))

        prev = _snap(eng)
        for k in range(3):
            if comm == "xgmi":
                eng.run(B, 1)  # graph-captured: step, reduction, all-reduce (sum only), optimiser pass
            else:
                eng.run_external(B, 1, allreduce)
            cur = _snap(eng)
            # engine.grads holds the gradient summed over the ranks (CC4 tail included); the update averages it
            _check_update(prev, cur, TABLE[k], inv_ws=1.0 / ws, tag=f"rank {rank} {comm} step {k}")
            assert cur["step"] == k + 1
            for key in ("params", "buf", "grads"):
                other = cur[key].clone()
                dist.broadcast(other, 0)
                assert torch.equal(cur[key], other), (key, k)
            prev = cur
        eng.check_errors()
        assert eng.read_loss()[1] == 3
        if tr is not None:
            tr.close()
        else:
            dist.barrier()
            eng.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("comm", ["xgmi", "external"])
@pytest.mark.parametrize("dtype,persistent", [("bf16", True), ("fp32", False)], ids=["sliced", "multikernel"])
def test_two_ranks_one_gpu(gpu, port, dtype, persistent, comm):
    spawn_ranks(_rank_worker, 2, lambda r: (r, 2, port, dtype, persistent, comm))


# ---- entry point ---------------------------------------------------------------------------------------------------
def test_main_entry_point_with_optimizer_flags(gpu, tmp_path):
    mj = tmp_path / "m.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "main.py", "--world-size", "1", "--synthetic", "512", "--epochs", "2",
                        "--max-steps", "8", "--momentum", "0.9", "--lr-schedule", "cosine", "--eval", "--port",
                        str(free_port()), "--checkpoint-path", str(tmp_path / "birds_vs_airplanes.pt"),
                        "--metrics-json", str(mj)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Epoch 1, Training loss \d", r.stdout) and "Test accuracy" in r.stdout, r.stdout
    from distributeddataparallel_cifar10_amd.utils.schedule import lr_table
    table = lr_table("cosine", 1e-2, 16)
    recs = [x for x in map(json.loads, mj.read_text().splitlines()) if "epoch" in x]
    assert [x["steps"] for x in recs] == [8, 8] and all(np.isfinite(x["loss"]) and x["loss"] > 0 for x in recs)
    assert [x["lr"] for x in recs] == [table[7], table[15]]
    assert sorted(os.listdir(tmp_path)) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.meta.json",
                                            "birds_vs_airplanes.pt.optim.pt", "m.json"]
    assert len(torch.load(str(tmp_path / "birds_vs_airplanes.pt"), weights_only=True)) == 66


def _main_flow(tmp, name, **kw):
    """main.py's per-rank flow at world size 1 (loader, build_model_for_rank, train_loop) with --synthetic 512
    --max-steps 8 --momentum 0.9 --lr-schedule cosine; writes the final state as a checkpoint and returns its path
    and the final momentum buffers."""
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint
    dev = torch.device("cuda", 0)
    cfg = TrainConfig(synthetic=512, epochs=2, max_steps=8, momentum=0.9, lr_schedule="cosine", **kw)
    data, labels = load_dataset(cfg)
    loader = DeviceLoader(data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=dev,
                          sampler="distributed", seed=0, set_epoch=cfg.set_epoch)
    torch.manual_seed(21)
    model = build_model_for_rank(cfg, 0, 1, dev, data, labels, loader)
    try:
        try:
            train_loop(model, loader, 0, cfg)
        except RuntimeError as ex:
            if "injected failure" not in str(ex):
                raise
        bufs = {k: v.detach().cpu().clone() for k, v in model.engine.optimizer_state()["momentum_buffer"].items()}
        final = save_checkpoint(model, os.path.join(tmp, name + "_final.pt"), 0)
    finally:
        model.close()
    return final, bufs


def test_resume_gives_the_same_checkpoint(gpu, tmp_path):
    """Two epochs straight against one epoch + --resume on the fused engine (momentum 0.9, cosine over both epochs; the
    first leg is the 2-epoch run stopped after its first epoch, so both legs share one table): bitwise equal final
    checkpoint and momentum buffers."""
    tmp = str(tmp_path)
    a, bufs_a = _main_flow(tmp, "a", checkpoint_path=os.path.join(tmp, "a.pt"))
    leg = os.path.join(tmp, "b.pt")
    _main_flow(tmp, "b1", checkpoint_path=leg, fail_at_step=9)  # epoch 1 (8 steps, checkpoint), stopped at step 9
    assert json.load(open(leg + ".meta.json")) == {"epoch": 1, "step": 8, "opt_step": 8}
    b, bufs_b = _main_flow(tmp, "b2", resume=leg, checkpoint=False)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for k in bufs_a:
        assert torch.equal(bufs_a[k], bufs_b[k]), k
