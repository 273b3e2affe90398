"""The EMA form of the fused engine's optimiser pass (csrc/optimizer.hip ``k_apply_opt<BF, true>``) on an MI355X: every
update against the float64 oracle ``utils/ema.ema_reference``, the run without EMA (bitwise), decay 0 with a poisoned
tail, graph replay, evaluation of the averaged model, two ranks on one GPU, and the entry point with resume.

All cases: 256 synthetic images, batch 8 (the pass's size is the fixed 76,140-float buffer; its last workgroup is
ragged: 19,019 float4 over 75 x 256 threads).  Tolerance of an update: <= 1e-6 relative L2 per tensor (one fp32 subtract
and one fused multiply-add, with the decay rounded to fp32, against float64: 3.3e-8 for decays 0 to 0.9999 on the CPU;
measured here <= 4.2e-8)."""
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
DECAY = 0.3  # with warm-up the first three updates use 1/10, 2/11, 3/12 and the cap holds from the fourth (4/13 > 0.3)
NDATA, B = 256, 8
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}
TOL = 1e-6
OFF_RS = 76076


def _opt(decay=DECAY, warmup=False):
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    return OptimizerConfig(momentum=MU, weight_decay=WD, lr_table=TABLE, ema_decay=decay, ema_warmup=warmup)


def _engine(dtype, persistent, optimizer, seed=11, **kw):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    dev = torch.device("cuda", 0)
    data, labels = synthetic_cifar(NDATA, seed=3)
    torch.manual_seed(seed)
    model = NetResDeep().to(dev)
    eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                           EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, optimizer=optimizer, **kw))
    eng.set_indices(list(range(NDATA)))
    eng.set_cursor(0)
    eng.read_loss(reset=True)
    return model, eng


def _snap(eng):
    eng.sync()
    torch.cuda.synchronize()
    return dict(params=eng.flat.detach().cpu().clone(), buf=eng.momentum.detach().cpu().clone(),
                ema=None if eng.ema is None else eng.ema.detach().cpu().clone(),
                rs=torch.cat([eng.bn.running_mean, eng.bn.running_var]).detach().cpu().clone(),
                step=eng.optimizer_step(), loss=eng.read_loss()[0])


@functools.lru_cache(maxsize=None)
def _eager_steps(kind, decay, warmup):
    """Five single eager steps; the state before and after every step.  decay None: the same run without EMA."""
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(decay, warmup))
    assert eng.kind_name == ("sliced" if persistent else "multikernel")
    assert (eng.ema is None) == (decay is None)
    snaps = [_snap(eng)]
    for _ in range(5):
        eng.run(B, 1, graph=False)
        snaps.append(_snap(eng))
    eng.check_errors()
    eng.close()
    return snaps


def _check_update(prev, cur, d, tag=""):
    """cur's average = ema_reference(prev's average, cur's parameters / running statistics, d), per tensor."""
    from distributeddataparallel_cifar10_amd.runtime.engine import LAYOUT
    from distributeddataparallel_cifar10_amd.utils.ema import ema_reference
    worst = 0.0
    parts = {name: (slice(off, off + int(np.prod(shape))), cur["params"]) for name, (off, shape) in LAYOUT.items()}
    for name, (sl, src) in parts.items():
        want = ema_reference(prev["ema"][sl], src[sl], d)
        err = float(np.linalg.norm(cur["ema"][sl].double().numpy() - want) / max(np.linalg.norm(want), 1e-300))
        worst = max(worst, err)
        assert err <= TOL, (tag, name, err)
    rs = slice(OFF_RS, OFF_RS + 64)
    want = ema_reference(prev["ema"][rs], cur["rs"], d)
    err = float(np.linalg.norm(cur["ema"][rs].double().numpy() - want) / np.linalg.norm(want))
    worst = max(worst, err)
    print(f"{tag}: d = {d:.6f}, worst relative L2 {worst:.3e} (running statistics {err:.3e})")
    assert err <= TOL, (tag, "running statistics", err)


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("kind", list(ENGINES))
def test_per_update_matches_reference(gpu, kind, warmup):
    from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at
    snaps = _eager_steps(kind, DECAY, warmup)
    s0 = snaps[0]  # the average starts as a copy of the model
    assert torch.equal(s0["ema"][:OFF_RS], s0["params"][:OFF_RS])
    assert torch.equal(s0["ema"][OFF_RS:OFF_RS + 64], s0["rs"])
    for k in range(5):
        assert not torch.equal(snaps[k + 1]["rs"], snaps[k]["rs"])  # the step moved the statistics
        _check_update(snaps[k], snaps[k + 1], ema_decay_at(k, DECAY, warmup), tag=f"{kind} step {k}")
        assert snaps[k + 1]["step"] == k + 1
    if warmup:  # the two runs differ exactly while the warm-up value is below the cap
        plain = _eager_steps(kind, DECAY, False)
        assert not torch.equal(snaps[5]["ema"], plain[5]["ema"])


@pytest.mark.parametrize("kind", list(ENGINES))
def test_training_is_bitwise_the_run_without_ema(gpu, kind):
    with_ema, without = _eager_steps(kind, DECAY, True), _eager_steps(kind, None, False)
    for k in range(6):
        for key in ("params", "buf", "rs"):
            assert torch.equal(with_ema[k][key], without[k][key]), (k, key)
        assert with_ema[k]["loss"] == without[k]["loss"] and with_ema[k]["step"] == without[k]["step"] == k


@pytest.mark.parametrize("kind", list(ENGINES))
def test_decay_zero_copies_the_model_and_keeps_the_tail(gpu, kind):
    """Decay 0: the average is the model bit for bit after every step -- all 19,019 float4 of the ragged sweep and the
    64 statistics -- and nothing beyond OFF_RS + 64 is written (the tail is pre-filled with NaN)."""
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(0.0, True))
    eng.ema[OFF_RS + 64:].fill_(float("nan"))
    eng.ema[:OFF_RS + 64].fill_(123.0)  # (not the model: every element has to be written by the pass)
    torch.cuda.synchronize()
    tail = eng.ema.numel() - (OFF_RS + 64)
    assert tail == 20
    for k in range(5):
        eng.run(B, 1, graph=False)
        s = _snap(eng)
        assert torch.equal(s["ema"][:OFF_RS], s["params"][:OFF_RS]), k
        assert torch.equal(s["ema"][OFF_RS:OFF_RS + 64], s["rs"]), k
        assert bool(torch.isnan(s["ema"][OFF_RS + 64:]).all()), k
    eng.close()


@pytest.mark.parametrize("kind", list(ENGINES))
def test_graph_replay_equals_eager_steps(gpu, kind):
    """One 4-step graph replay is bitwise the four eager steps, average included (the decay, the warm-up flag and the
    step are read from device memory inside the captured graph); set_ema_decay between two replays of the same graph
    takes effect: with decay 0 the average becomes the model."""
    snaps = _eager_steps(kind, DECAY, True)
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(DECAY, True))
    eng.run(B, 4, graph=True)
    got = _snap(eng)
    assert got["step"] == 4 and got["loss"] == snaps[4]["loss"]
    for key in ("params", "buf", "ema", "rs"):
        assert torch.equal(got[key], snaps[4][key]), key
    assert not torch.equal(got["ema"][:OFF_RS], got["params"][:OFF_RS])
    eng.set_ema_decay(0.0)
    assert eng.cfg.optimizer.ema_decay == 0.0 and eng.cfg.optimizer.ema_warmup is True
    eng.run(B, 4, graph=True)
    after = _snap(eng)
    eng.close()
    assert after["step"] == 8
    assert torch.equal(after["ema"][:OFF_RS], after["params"][:OFF_RS])
    assert torch.equal(after["ema"][OFF_RS:OFF_RS + 64], after["rs"])


@pytest.mark.parametrize("kind", ["sliced-bf16", "sliced-fp32"])
def test_evaluate_ema(gpu, kind):
    """engine.evaluate(ema=True): bitwise evaluate_netresdeep on a fresh model loaded from ema_state_dict(); after
    training steps not the live model's result; the call changes neither the parameters nor the average."""
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_netresdeep
    dtype, persistent = ENGINES[kind]
    _, eng = _engine(dtype, persistent, _opt(0.9, False))
    eng.run(B, 6)
    before = _snap(eng)
    avg = eng.evaluate(ema=True)
    live = eng.evaluate()
    after = _snap(eng)
    for key in ("params", "buf", "ema", "rs"):
        assert torch.equal(before[key], after[key]), key
    sd = eng.ema_state_dict()
    assert len(sd) == 66 and list(sd) == list(NetResDeep().state_dict())
    assert int(sd["resblocks.0.batch_norm.num_batches_tracked"]) == 60
    assert sd["resblocks.3.conv.weight"].data_ptr() == sd["resblocks.0.conv.weight"].data_ptr()
    fresh = NetResDeep()
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    fresh = fresh.to(eng.device)
    want = evaluate_netresdeep(fresh, eng.data, eng.labels, dtype=dtype)
    assert avg.count == want.count == NDATA
    assert torch.equal(avg.pred, want.pred) and torch.equal(avg.loss, want.loss)
    assert avg.loss_sum == want.loss_sum
    assert not torch.equal(avg.loss, live.loss)
    # the state round-trips
    keep = {k: v.detach().cpu().clone() for k, v in sd.items()}
    eng.reset_ema()
    s = _snap(eng)
    assert torch.equal(s["ema"][:OFF_RS], s["params"][:OFF_RS]) and torch.equal(s["ema"][OFF_RS:OFF_RS + 64], s["rs"])
    eng.load_ema_state_dict(keep)
    assert torch.equal(_snap(eng)["ema"][:OFF_RS + 64], before["ema"][:OFF_RS + 64])
    with pytest.raises(ValueError):
        eng.load_ema_state_dict({"fc1.weight": keep["fc1.weight"]})
    eng.close()


def test_ema_off_allocates_nothing_and_keeps_the_plan(gpu):
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    _, plain = _engine("bf16", True, None)
    assert plain.ema is None
    with pytest.raises(RuntimeError, match="no optimiser"):
        plain.set_ema_decay(0.9)
    with pytest.raises(RuntimeError, match="no EMA"):
        plain.evaluate(ema=True)
    plain.close()
    _, off = _engine("bf16", True, OptimizerConfig(momentum=MU, weight_decay=WD, lr_table=TABLE))
    _, on = _engine("bf16", True, _opt())
    assert off.ema is None and on.ema is not None and tuple(on.ema.shape) == (76160,)
    for batch in (B, 3, 1):
        a, b = off.step_plan(batch), on.step_plan(batch)
        assert [getattr(a, f) for f, _ in a._fields_] == [getattr(b, f) for f, _ in b._fields_]
    with pytest.raises(ValueError):
        on.set_ema_decay(1.0)
    from distributeddataparallel_cifar10_amd.runtime import native
    assert on.lib.dca_engine_set_ema(on.h, on.ema.data_ptr() + 4, 0.5, 0) == -1  # refused before anything changes
    assert "16-byte aligned" in native.last_error()
    assert on.lib.dca_engine_set_ema(on.h, on.ema.data_ptr(), 1.0, 0) == -1 and "[0, 1)" in native.last_error()
    on.set_ema_decay(None)  # off again: the buffer is gone, the pass runs in its plain form
    assert on.ema is None and on.cfg.optimizer.ema_decay is None
    on.run(B, 2)
    off.run(B, 2)
    assert torch.equal(_snap(on)["params"], _snap(off)["params"])
    off.close()
    on.close()


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
        from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at
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
                                 comm="xgmi", max_indices=len(order), optimizer=_opt(DECAY, True))
            assert tr.comm == "xgmi", tr.comm
            eng = tr.engine
        else:
            eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                                   EngineConfig(batch_max=B, dtype=dtype, persistent=persistent, world_size=ws,
                                                rank=rank, comm="external", optimizer=_opt(DECAY, True)))
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
                eng.run(B, 1)  # graph-captured: step, reduction, all-reduce (sum only), optimiser pass with EMA
            else:
                eng.run_external(B, 1, allreduce)
            cur = _snap(eng)
            _check_update(prev, cur, ema_decay_at(k, DECAY, True), tag=f"rank {rank} {comm} step {k}")
            assert cur["step"] == k + 1
            for key, sl in (("params", slice(0, OFF_RS)), ("ema", slice(0, OFF_RS))):
                other = cur[key][sl].clone()
                dist.broadcast(other, 0)
                assert torch.equal(cur[key][sl], other), (key, k)
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
def test_main_entry_point_with_ema_flags(gpu, tmp_path):
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.utils.ema import ema_decay_at
    mj = tmp_path / "m.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "main.py", "--world-size", "1", "--synthetic", "512", "--epochs", "2",
                        "--max-steps", "8", "--momentum", "0.9", "--ema-decay", "0.99", "--ema-warmup", "--eval",
                        "--port", str(free_port()), "--checkpoint-path", str(tmp_path / "birds_vs_airplanes.pt"),
                        "--metrics-json", str(mj)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Epoch 1, Training loss \d", r.stdout), r.stdout
    lines = re.findall(r"Epoch (\d+), EMA test accuracy (\d\.\d{4}), EMA test loss (\S+)", r.stdout)
    assert [ln[0] for ln in lines] == ["1", "2"], r.stdout
    assert len(re.findall(r"Epoch \d+, Test accuracy", r.stdout)) == 2
    recs = [x for x in map(json.loads, mj.read_text().splitlines()) if "epoch" in x]
    assert [x["steps"] for x in recs] == [8, 8]
    assert [x["ema_decay"] for x in recs] == [ema_decay_at(7, 0.99, True), ema_decay_at(15, 0.99, True)]
    for x, ln in zip(recs, lines):
        assert "{:.4f}".format(x["ema_eval_accuracy"]) == ln[1] and repr(x["ema_eval_loss"]) == ln[2]
        assert np.isfinite(x["ema_eval_loss"]) and x["ema_eval_loss"] != x["eval_loss"]
    assert sorted(os.listdir(tmp_path)) == ["birds_vs_airplanes.pt", "birds_vs_airplanes.pt.ema.pt",
                                            "birds_vs_airplanes.pt.meta.json", "birds_vs_airplanes.pt.optim.pt",
                                            "m.json"]
    avg = torch.load(str(tmp_path / "birds_vs_airplanes.pt.ema.pt"), weights_only=True)
    assert len(avg) == 66
    NetResDeep().load_state_dict(avg, strict=True)
    live = torch.load(str(tmp_path / "birds_vs_airplanes.pt"), weights_only=True)
    assert not torch.equal(avg["fc1.weight"], live["fc1.weight"])
    assert torch.equal(avg["resblocks.0.batch_norm.num_batches_tracked"],
                       live["resblocks.0.batch_norm.num_batches_tracked"])


def _main_flow(tmp, name, **kw):
    """main.py's per-rank flow at world size 1 (loader, build_model_for_rank, train_loop) with --synthetic 512
    --max-steps 8 --momentum 0.9 --lr-schedule cosine --ema-decay 0.9 --ema-warmup; writes the final state as a
    checkpoint and returns its path, the final momentum buffers and the final average."""
    from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader
    from distributeddataparallel_cifar10_amd.train import TrainConfig, build_model_for_rank, load_dataset, train_loop
    from distributeddataparallel_cifar10_amd.utils.checkpoint import save_checkpoint
    dev = torch.device("cuda", 0)
    cfg = TrainConfig(synthetic=512, epochs=2, max_steps=8, momentum=0.9, lr_schedule="cosine", ema_decay=0.9,
                      ema_warmup=True, **kw)
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
        avg = {k: v.detach().cpu().clone() for k, v in model.engine.ema_state_dict().items()}
        final = save_checkpoint(model, os.path.join(tmp, name + "_final.pt"), 0)
    finally:
        model.close()
    return final, bufs, avg


def test_resume_gives_the_same_checkpoint_and_average(gpu, tmp_path):
    """Two epochs straight against one epoch + --resume on the fused engine: bitwise equal final checkpoint, momentum
    buffers and average; the first leg's .ema.pt is the average at its checkpoint."""
    tmp = str(tmp_path)
    a, bufs_a, avg_a = _main_flow(tmp, "a", checkpoint_path=os.path.join(tmp, "a.pt"))
    leg = os.path.join(tmp, "b.pt")
    _main_flow(tmp, "b1", checkpoint_path=leg, fail_at_step=9)  # epoch 1 (8 steps, checkpoint), stopped at step 9
    assert json.load(open(leg + ".meta.json")) == {"epoch": 1, "step": 8, "opt_step": 8}
    assert len(torch.load(leg + ".ema.pt", weights_only=True)) == 66
    b, bufs_b, avg_b = _main_flow(tmp, "b2", resume=leg, checkpoint=False)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert list(sa) == list(sb) and len(sa) == 66
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(avg_a[k], avg_b[k]), k
    for k in bufs_a:
        assert torch.equal(bufs_a[k], bufs_b[k]), k
    assert not torch.equal(avg_a["fc1.weight"], sa["fc1.weight"])
