"""The crop + flip pass on an MI355X (csrc/augment.hip: k_augment_u8) against the definition (data/augment.py), bit for
bit; its C ABI's argument checks; and the fused trainers on an augmenting loader against plain trainers fed the
reference's images, bitwise (64 synthetic images, batch 8, 2 epochs of 4 steps)."""
import ctypes

import numpy as np
import pytest
import torch

from distributeddataparallel_cifar10_amd.data.augment import AugmentConfig, augment_reference, augment_u8
from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _images(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g)


def _check(dev, n, ids, seed=0, epoch=1, pad=4, flip=True, stream=None, sync=None):
    """The kernel on `n` random images into a dst pre-filled with 0xA5 == the reference into the same."""
    src = _images(n, seed=n)
    want = augment_reference(src, ids, seed, epoch, pad, flip, out=torch.full_like(src, FILL))
    d_src = src.to(dev)
    dst = torch.full_like(d_src, FILL)
    assert augment_u8(d_src, dst, ids, seed=seed, epoch=epoch, pad=pad, flip=flip, stream=stream) is dst
    (sync or torch.cuda.synchronize)()
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)
    assert torch.equal(d_src.cpu(), src)
    return want


# ---- the kernel ---------------------------------------------------------------------------------------------------
def test_every_cell_4096_images(gpu):
    """ids=None, seed 0, epoch 8, N = 4,096: all 162 (dy, dx, f) cells occur (tests/test_augment.py)."""
    _check(gpu, 4096, None, seed=0, epoch=8)


@pytest.mark.parametrize("pad", [0, 1, 4, 8])
@pytest.mark.parametrize("flip", [True, False])
def test_pads_and_flip(gpu, pad, flip):
    want = _check(gpu, 64, None, seed=12345, epoch=3, pad=pad, flip=flip)
    if pad == 0 and not flip:
        assert torch.equal(want, _images(64, seed=64))


def test_id_lists(gpu):
    _check(gpu, 64, [37])                                              # one id
    _check(gpu, 256, np.random.default_rng(0).permutation(256)[:193])  # 193 images: the last workgroup is half empty
    _check(gpu, 64, [5, 9, 5, 63, 9, 5, 0, 0])                         # duplicates write identical bytes
    want = _check(gpu, 300, np.arange(1, 300, 7), seed=1, epoch=2)     # a strided subset ...
    rest = np.setdiff1d(np.arange(300), np.arange(1, 300, 7))
    assert bool((want[rest] == FILL).all())                            # ... the other rows keep 0xA5
    _check(gpu, 64, torch.tensor([3, 1, 2], device=gpu))               # ids as a device tensor


def test_streams(gpu):
    """A torch stream and a raw hipStream_t (the engine's own) both work."""
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    side = torch.cuda.Stream(gpu)
    _check(gpu, 64, None, stream=side, sync=side.synchronize)
    data, labels = synthetic_cifar(64, seed=3)
    eng = NetResDeepEngine(NetResDeep().to(gpu), data.to(gpu), labels.to(gpu), EngineConfig(batch_max=8))
    try:
        raw = eng.lib.dca_engine_stream(eng.h)
        assert isinstance(raw, int) and raw
        _check(gpu, 64, [1, 2, 3, 60], stream=raw, sync=eng.sync)
    finally:
        eng.close()


# ---- the C ABI refuses bad arguments without launching ------------------------------------------------------------
def test_c_abi_validation(gpu):
    from distributeddataparallel_cifar10_amd.runtime import native
    lib = native.require_native()
    src = _images(8).to(gpu)
    dst = torch.full_like(src, FILL)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(src_p=src.data_ptr(), dst_p=dst.data_ptr(), n=8, n_rows=8, pad=4):
        return lib.dca_augment_u8(src_p, dst_p, None, n, n_rows, 0, 1, pad, 1, st)

    for kw, word in (({"n_rows": 0}, "n_rows"), ({"pad": 9}, "pad"), ({"pad": -1}, "pad"), ({"n": 9}, "n must"),
                     ({"n": -1}, "n must"), ({"src_p": None}, "null"), ({"dst_p": src.data_ptr() + 3072}, "overlap"),
                     ({"src_p": src.data_ptr() + 4}, "aligned")):
        assert call(**kw) == -1, kw
        assert word in lib.dca_augment_last_error().decode(), (kw, lib.dca_augment_last_error())
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())  # nothing was launched
    with pytest.raises(ValueError, match="out of range"):
        augment_u8(src, dst, [0, 8], seed=0, epoch=1)  # an id out of range never reaches the device
    with pytest.raises(ValueError):
        augment_u8(src, dst, seed=0, epoch=1, pad=9)
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), augment_reference(src.cpu(), None, 0, 1))


# ---- fused trainers -----------------------------------------------------------------------------------------------
NDATA, B, STEPS, SEED = 64, 8, 4, 21
ENGINES = {"sliced-bf16": ("bf16", True), "sliced-fp32": ("fp32", True), "multikernel-fp32": ("fp32", False)}


def _trainer(dev, dtype, persistent, augment):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.parallel.ddp import FusedDDPTrainer
    from distributeddataparallel_cifar10_amd.train import eval_source
    data, labels = synthetic_cifar(NDATA, seed=3)
    uploaded = data.to(dev)
    # (the plain twin gets a tensor of its own: the test rewrites it between epochs)
    loader = DeviceLoader(uploaded if augment else uploaded.clone(), labels, batch_size=B, device=dev, augment=augment)
    torch.manual_seed(11)
    model = NetResDeep().to(dev)
    tr = FusedDDPTrainer(model, loader.data, loader.labels, batch_max=B, dtype=dtype, persistent=persistent,
                         max_indices=NDATA, **eval_source(loader))
    return data, labels, uploaded, loader, model, tr


@pytest.mark.parametrize("kind", list(ENGINES))
def test_trainer_on_augmenting_loader_is_bitwise_the_plain_one_on_reference_images(gpu, kind):
    dtype, persistent = ENGINES[kind]
    src, labels, up_a, la, ma, ta = _trainer(gpu, dtype, persistent, AugmentConfig(seed=SEED))
    _, _, _, lb, mb, tb = _trainer(gpu, dtype, persistent, None)
    try:
        assert ta.engine.kind_name == tb.engine.kind_name == kind.split("-")[0]
        assert la.source.data_ptr() == up_a.data_ptr() and ta.engine.data.data_ptr() == la.data.data_ptr()
        assert ta.engine.eval_data.data_ptr() == la.source.data_ptr()
        stream = ta.engine.lib.dca_engine_stream(ta.engine.h)
        # evaluate() of the augmented trainer reads the pristine images (checked on the initial model, whose logits
        # depend on the image, with the first epoch's crops already in `data`)
        la.set_epoch(1)
        la.augment_epoch(None, stream=stream)
        own = ta.engine.evaluate()
        pristine = ta.engine.evaluate(up_a, la.labels)
        assert (own.correct, own.count, own.loss_sum) == (pristine.correct, pristine.count, pristine.loss_sum)
        assert torch.equal(own.loss, pristine.loss) and torch.equal(own.pred, pristine.pred)
        assert not torch.equal(own.loss, ta.engine.evaluate(la.data, la.labels).loss)
        for epoch in (1, 2):
            for ld in (la, lb):
                ld.set_epoch(epoch)
            idx = la.indices()[:STEPS * B]
            assert np.array_equal(idx, lb.indices()[:STEPS * B])
            # A: the pass on the engine's stream, as train_loop issues it
            la.augment_epoch(idx, stream=stream)
            loss_a = ta.engine.run_epoch(idx, B)
            # B: the plain trainer reads the reference's images of this epoch
            want = augment_reference(src, None, SEED, epoch)
            tb.engine.sync()
            lb.data.copy_(want.to(gpu))
            torch.cuda.synchronize()
            loss_b = tb.engine.run_epoch(idx, B)
            assert loss_a == loss_b and loss_a[1] == STEPS, (epoch, loss_a, loss_b)
            sa, sb = ma.state_dict(), mb.state_dict()
            assert list(sa) == list(sb)
            for name in sa:
                assert torch.equal(sa[name], sb[name]), (epoch, name)
            rows = torch.from_numpy(np.unique(idx))
            assert torch.equal(la.data.cpu()[rows], want[rows])
            assert torch.equal(la.source.cpu(), src)
        assert not torch.equal(la.data.cpu(), src)
    finally:
        ta.close()
        tb.close()


def test_default_allocates_no_second_dataset(gpu):
    _, _, uploaded, loader, _, tr = _trainer(gpu, "bf16", True, None)
    try:
        up = loader.data  # (_trainer cloned the upload for the plain twin; the loader must not clone again)
        again = DeviceLoader(up, loader.labels, batch_size=B, device=gpu)
        assert again.augment is None and not hasattr(again, "source")
        assert again.data.data_ptr() == up.data_ptr()
        assert tr.engine.data.data_ptr() == up.data_ptr() and tr.engine.eval_data is tr.engine.data
        before = torch.cuda.memory_allocated(gpu)
        again.set_epoch(1)
        again.augment_epoch(again.indices())
        assert torch.cuda.memory_allocated(gpu) == before
    finally:
        tr.close()
