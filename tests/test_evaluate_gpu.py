"""The fused eval-mode NetResDeep kernel (csrc/netresdeep_eval.hip) on the GPU: logits and predictions against the
CPU oracle ``reference_eval``, exact self-consistency of the per-image outputs, bitwise grid independence, index
gathering, the engine integration (``NetResDeepEngine.evaluate`` reads, never writes) and two ranks on one device.

Fixture of the oracle comparisons: ``synthetic_cifar(1312, seed=5, learnable=True)``, ``torch.manual_seed(1)``, 200
stock SGD steps (lr 1e-2, batch 32) over the first 1024 images on the CPU, evaluation on images 1024 .. 1311 -- the
BatchNorm running statistics are then far from their initial values.
"""
import copy
import os
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from _ranks import spawn_ranks

pytestmark = pytest.mark.gpu

N_TRAIN, N_ALL = 1024, 1312
# bounds on the relative L2 error of the logits (the project's bounds, tests/test_engine_gpu.py): fp32 mode against
# the fp32 oracle; bf16 mode against the fp32 oracle (an independent forward) and against the oracle with the same
# operand rounding (arithmetic only)
FP32_REL, BF16_REL, BF16_ARITH_REL = 1e-4, 5e-2, 3e-3
# predictions are compared where the fp32 oracle's margin (top1 - top2) / max|logit| exceeds this
MARGIN = {"fp32": 1e-3, "bf16": 5e-2}
MAX_LEFT_OUT = 0.10


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _decided(oracle, dtype):
    top = oracle.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) / oracle.abs().max(dim=1).values > MARGIN[dtype]


@pytest.fixture(scope="module")
def fx(gpu):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.utils.oracle import normalize_u8, reference_eval
    data, labels = synthetic_cifar(N_ALL, seed=5, learnable=True)
    torch.manual_seed(1)
    model = NetResDeep()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    for s in range(200):
        sel = slice(32 * (s % 32), 32 * (s % 32) + 32)
        opt.zero_grad()
        F.cross_entropy(model(normalize_u8(data[sel])), labels[sel]).backward()
        opt.step()
    held = torch.arange(N_TRAIN, N_ALL)
    return {
        "cpu": model, "gpu": copy.deepcopy(model).to(gpu), "data": data.to(gpu), "labels": labels.to(gpu),
        "held": held, "labels_cpu": labels,
        "oracle": reference_eval(model, data[held]),
        "oracle_bf16": reference_eval(model, data[held], bf16_operands=True, fc1_bf16=True),
    }


def _eval(fx, dtype, idx=None, **kw):
    from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_netresdeep
    idx = fx["held"] if idx is None else idx
    return evaluate_netresdeep(fx["gpu"], fx["data"], fx["labels"], indices=idx, dtype=dtype, return_logits=True, **kw)


@pytest.mark.parametrize("n", [1, 37, 288])
def test_logits_against_the_oracle(fx, n):
    fp32 = _eval(fx, "fp32", fx["held"][:n]).logits.cpu()
    bf16 = _eval(fx, "bf16", fx["held"][:n]).logits.cpu()
    e32, e16, e16a = _rel(fp32, fx["oracle"][:n]), _rel(bf16, fx["oracle"][:n]), _rel(bf16, fx["oracle_bf16"][:n])
    print(f"n={n}: fp32 vs oracle {e32:.3e}; bf16 vs oracle {e16:.3e}; bf16 vs bf16-operand oracle {e16a:.3e}")
    assert e32 <= FP32_REL
    assert e16 <= BF16_REL
    assert e16a <= BF16_ARITH_REL


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predictions_against_the_oracle(fx, dtype):
    res = _eval(fx, dtype)
    keep = _decided(fx["oracle"], dtype)
    left_out = 1.0 - float(keep.double().mean())
    print(f"{dtype}: {left_out:.3%} of the images left out by the margin rule")
    assert left_out <= MAX_LEFT_OUT
    assert torch.equal(res.pred.cpu().long()[keep], fx["oracle"].argmax(1)[keep])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_outputs_are_self_consistent(fx, dtype):
    from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_netresdeep
    res = _eval(fx, dtype)
    logits, want = res.logits.cpu(), fx["labels_cpu"][fx["held"]]
    # argmax with ties to the lowest index, spelled out
    first_max = (logits == logits.max(1, keepdim=True).values).int().argmax(1)
    assert torch.equal(res.pred.cpu().long(), first_max)
    assert res.correct == int((first_max == want).sum()) and res.count == len(want)
    # the loss of every image, recomputed in float64 from the returned fp32 logits
    ref = torch.logsumexp(logits.double(), 1) - logits.double().gather(1, want[:, None])[:, 0]
    err = ((res.loss.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-12)).max()
    print(f"{dtype}: worst relative error of a per-image loss {float(err):.3e}")
    assert float(err) <= 1e-6
    assert res.loss_sum == float(res.loss.double().sum())
    # without return_logits: the same sums, no logits
    plain = evaluate_netresdeep(fx["gpu"], fx["data"], fx["labels"], indices=fx["held"], dtype=dtype)
    assert plain.logits is None and (plain.correct, plain.loss_sum) == (res.correct, res.loss_sum)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_grid_independence_is_bitwise(fx, dtype):
    idx = fx["held"][:37]
    runs = [_eval(fx, dtype, idx, max_workgroups=g) for g in (1, 8, 0, 0)]
    for r in runs[1:]:
        assert torch.equal(r.logits, runs[0].logits) and torch.equal(r.pred, runs[0].pred)
        assert (r.correct, r.loss_sum) == (runs[0].correct, runs[0].loss_sum)
    # one workgroup walking 37 images with its resident weights = 37 separate launches
    singles = torch.cat([_eval(fx, dtype, idx[k:k + 1]).logits for k in (0, 1, 36)])
    assert torch.equal(singles, runs[0].logits[[0, 1, 36]])


def test_index_gather(fx):
    plain = _eval(fx, "bf16", torch.arange(N_ALL - 40, N_ALL))
    for order in (list(range(N_ALL - 1, N_ALL - 41, -1)), [N_ALL - 1, 0, N_ALL - 1, N_ALL - 40, 0]):
        res = _eval(fx, "bf16", order)
        whole = {N_ALL - 40 + k: plain.logits[k] for k in range(40)}
        whole[0] = _eval(fx, "bf16", [0]).logits[0]
        assert torch.equal(res.logits, torch.stack([whole[i] for i in order]))
        assert res.count == len(order)
    for bad in ([0, N_ALL], [-1], [2 ** 31]):
        with pytest.raises(ValueError):
            _eval(fx, "bf16", bad)


def _engine(gpu, dtype, persistent, n_data=256, repeats=1):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    data, labels = synthetic_cifar(n_data, seed=5, learnable=True)
    torch.manual_seed(7)
    model = NetResDeep().to(gpu)
    eng = NetResDeepEngine(model, data.to(gpu), labels.to(gpu),
                           EngineConfig(batch_max=32, dtype=dtype, persistent=persistent),
                           max_indices=n_data * repeats)
    eng.set_indices(list(range(n_data)) * repeats)
    eng.set_cursor(0)
    eng.read_loss(reset=True)
    return eng, model, data, labels


@pytest.mark.parametrize("dtype,persistent", [("bf16", True), ("fp32", True), ("fp32", False)])
def test_engine_evaluate_writes_nothing(gpu, dtype, persistent):
    from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_netresdeep
    states = []
    for with_eval in (False, True):
        eng, model, data, labels = _engine(gpu, dtype, persistent)
        assert eng.kind_name == ("sliced" if persistent else "multikernel")
        eng.run(32, 3)
        if with_eval:
            ev = eng.evaluate(return_logits=True)
            own = evaluate_netresdeep(eng.model, eng.data, eng.labels, dtype=dtype, return_logits=True)
            assert (ev.correct, ev.count, ev.loss_sum) == (own.correct, own.count, own.loss_sum) and ev.count == 256
            assert torch.equal(ev.logits, own.logits) and torch.equal(ev.pred, own.pred)
        eng.run(32, 3)
        loss, steps = eng.read_loss()
        states.append(({k: v.clone() for k, v in model.state_dict().items()}, loss, steps))
        eng.close()
    (a, la, sa), (b, lb, sb) = states
    assert sa == sb == 6 and la == lb
    assert int(a["resblocks.0.batch_norm.num_batches_tracked"]) == 60
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_engine_trained_model_accuracy(gpu):
    from distributeddataparallel_cifar10_amd.utils.oracle import reference_eval
    eng, model, data, labels = _engine(gpu, "bf16", True, repeats=25)
    eng.run(32, 200)
    ev = eng.evaluate()
    eng.sync()
    oracle = reference_eval(copy.deepcopy(model).cpu(), data)
    eng.close()
    keep = _decided(oracle, "bf16")
    print(f"engine-trained: {1 - float(keep.double().mean()):.3%} left out, accuracy {ev.accuracy:.4f}")
    assert 1.0 - float(keep.double().mean()) <= MAX_LEFT_OUT
    pred = ev.pred.cpu().long()
    assert torch.equal(pred[keep], oracle.argmax(1)[keep])
    assert int((pred[keep] == labels[keep]).sum()) == int((oracle.argmax(1)[keep] == labels[keep]).sum())
    assert ev.count == 256 and ev.correct == int((pred == labels).sum())


def _rank_worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=2)
        from distributeddataparallel_cifar10_amd.data.sampler import distributed_indices
        from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
        from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
        from distributeddataparallel_cifar10_amd.parallel.ddp import broadcast_module_state
        from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
        from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_distributed, evaluate_netresdeep
        dev = torch.device("cuda", 0)
        data, labels = synthetic_cifar(128, seed=5, learnable=True)
        torch.manual_seed(100 + rank)
        model = NetResDeep()
        broadcast_module_state(model, 0)
        model = model.to(dev)
        eng = NetResDeepEngine(model, data.to(dev), labels.to(dev),
                               EngineConfig(batch_max=32, dtype="bf16", persistent=True, world_size=2, rank=rank,
                                            comm="external"))
        eng.set_indices(distributed_indices(128, 2, rank))
        eng.set_cursor(0)

        def allreduce(t):
            h = t.cpu()
            dist.all_reduce(h)
            t.copy_(h.to(t.device))

        eng.run_external(16, 2, allreduce)
        idx = list(range(127))  # an odd count: the shards differ in length
        got = evaluate_distributed(model, eng.data, eng.labels, idx, evaluate=eng.evaluate)
        triple = [got.correct, got.count, got.loss_sum]
        # rank 0's state, all indices, one process
        want = [None]
        if rank == 0:
            one = evaluate_netresdeep(model, eng.data, eng.labels, idx, dtype="bf16")
            want = [[one.correct, one.count, one.loss_sum]]
        dist.broadcast_object_list(want, src=0)
        both = [None, None]
        dist.all_gather_object(both, triple)
        assert both[0] == both[1] == triple
        assert triple[:2] == want[0][:2] == [want[0][0], 127]
        assert triple[2] == pytest.approx(want[0][2], rel=1e-12)  # the same per-image losses, summed in two parts
        eng.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_on_one_device(gpu, port):
    spawn_ranks(_rank_worker, 2, lambda r: (r, port))
