"""Random-crop + flip augmentation (data/augment.py) on the CPU: the definition against an explicit construction, the
hash, the loader, the CLI and resume."""
import argparse
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributeddataparallel_cifar10_amd.data.augment import (AugmentConfig, augment_reference, augment_u8,
                                                              crop_flip_params)
from distributeddataparallel_cifar10_amd.data.loader import DeviceLoader

CPU = torch.device("cpu")


def _images(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g)


def _explicit(src, ids, seed, epoch, pad, flip):
    """pad, slice at (dy, dx), flip: torchvision's RandomCrop(32, padding=pad) + RandomHorizontalFlip, image by image."""
    dy, dx, f = crop_flip_params(seed, epoch, ids, pad, flip)
    out = src.clone()
    for k, i in enumerate(ids):
        p = F.pad(src[i], (pad, pad, pad, pad))
        crop = p[:, dy[k]:dy[k] + 32, dx[k]:dx[k] + 32]
        out[i] = crop.flip(-1) if f[k] else crop
    return out


# ---- the definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1, 4, 8])
@pytest.mark.parametrize("flip", [True, False])
def test_reference_equals_explicit_construction(pad, flip):
    src = _images(64, seed=pad)
    ids = list(range(64))
    dy, dx, f = crop_flip_params(3, 5, ids, pad, flip)
    assert dy.min() >= 0 and dy.max() <= 2 * pad and dx.min() >= 0 and dx.max() <= 2 * pad
    assert set(f.tolist()) <= ({0, 1} if flip else {0})
    got = augment_reference(src, None, 3, 5, pad, flip)
    assert got.dtype == torch.uint8 and torch.equal(got, _explicit(src, ids, 3, 5, pad, flip))
    assert torch.equal(augment_reference(src, ids, 3, 5, pad, flip), got)
    if pad:
        assert not torch.equal(got, src)


def test_rows_not_listed_stay_and_duplicates_are_harmless():
    src = _images(40)
    out = torch.full_like(src, 0xA5)
    ids = [3, 17, 3, 39, 17, 3]
    assert augment_reference(src, ids, 1, 2, out=out) is out
    want = _explicit(src, [3, 17, 39], 1, 2, 4, True)
    rest = [i for i in range(40) if i not in (3, 17, 39)]
    assert torch.equal(out[[3, 17, 39]], want[[3, 17, 39]])
    assert bool((out[rest] == 0xA5).all())
    dst = torch.full_like(src, 0xA5)
    assert augment_u8(src, dst, ids, seed=1, epoch=2) is dst  # the CPU path of the public entry: the reference
    assert torch.equal(dst, out)


def test_pad0_without_flip_is_identity():
    src = _images(16)
    assert torch.equal(augment_reference(src, None, 9, 4, pad=0, flip=False), src)
    dy, dx, f = crop_flip_params(9, 4, np.arange(16), pad=0, flip=True)
    assert not dy.any() and not dx.any()


# ---- the hash -----------------------------------------------------------------------------------------------------
def test_hand_computed_triples():
    """(dy, dx, f) worked out from the definition with plain integers, pad 4."""
    for (seed, epoch, i), want in {(0, 1, 0): (0, 4, 1), (12345, 8, 7): (7, 2, 1), (0, 3, 123): (5, 1, 0),
                                   (0, 8, 49999): (0, 8, 1)}.items():
        dy, dx, f = crop_flip_params(seed, epoch, [i])
        assert (int(dy[0]), int(dx[0]), int(f[0])) == want, (seed, epoch, i)


def _cells(seed, epoch, n):
    dy, dx, f = crop_flip_params(seed, epoch, np.arange(n))
    return np.bincount((dy * 9 + dx) * 2 + f, minlength=162)


def test_all_cells_occur_in_4096_ids():
    for epoch in range(1, 9):
        assert _cells(0, epoch, 4096).min() > 0, epoch


def test_chi_square_of_the_draws():
    """162 equiprobable (dy, dx, f) cells over ids 0..49,999: chi-square < 250 (p ~ 1e-5 at 161 degrees of freedom)
    for every seed and epoch checked."""
    worst = 0.0
    for seed in (0, 1, 12345):
        for epoch in range(1, 9):
            c = _cells(seed, epoch, 50000).astype(np.float64)
            e = 50000 / 162
            worst = max(worst, float(((c - e) ** 2 / e).sum()))
    assert worst < 250, worst
    a, b = crop_flip_params(0, 1, np.arange(50000)), crop_flip_params(0, 2, np.arange(50000))
    same = np.mean((a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2]))
    assert same < 0.01, same  # epochs draw independently (expected 1/162)


# ---- argument errors ----------------------------------------------------------------------------------------------
def test_augment_u8_argument_errors():
    src = _images(8)
    dst = torch.empty_like(src)
    for bad_src, bad_dst, kw in (
            (src.float(), dst, {}),                              # not uint8
            (src[:, :, :16], dst[:, :, :16], {}),                # not contiguous [N, 3, 32, 32]
            (src.reshape(8, 3, 16, 64), dst.reshape(8, 3, 16, 64), {}),
            (src, dst[:4], {}),                                  # shapes differ
            (src, src, {}),                                      # aliasing
            (src, dst, {"pad": 9}), (src, dst, {"pad": -1}),     # pad out of range
            (src, dst, {"ids": [0, 8]}), (src, dst, {"ids": [-1]})):
        with pytest.raises(ValueError):
            augment_u8(bad_src, bad_dst, kw.pop("ids", None), seed=0, epoch=1, **kw)
    both = _images(16)
    with pytest.raises(ValueError):
        augment_u8(both[:12], both[4:], seed=0, epoch=1)         # overlapping views
    with pytest.raises(ValueError):
        AugmentConfig(pad=9)


# ---- the loader ---------------------------------------------------------------------------------------------------
def _loader(n=96, **kw):
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    data, labels = synthetic_cifar(n, seed=3)
    return data, labels, DeviceLoader(data, labels, batch_size=32, device=CPU, **kw)


def test_loader_without_augment_is_todays():
    data, labels, ld = _loader()
    assert ld.augment is None and not hasattr(ld, "source")
    assert ld.data.data_ptr() == data.data_ptr()  # the uploaded tensor itself, no copy
    ld.augment_epoch()  # nothing to do
    assert torch.equal(ld.data, data)


def test_loader_with_augment():
    data, labels, ld = _loader(augment=AugmentConfig(seed=7))
    assert ld.source.data_ptr() == data.data_ptr() and ld.data.data_ptr() != data.data_ptr()
    assert torch.equal(ld.data, data)
    ptr = ld.data.data_ptr()
    epochs = []
    for epoch in (1, 2):
        ld.set_epoch(epoch)
        epochs.append(list(ld))
        assert torch.equal(ld.data, augment_reference(data, None, 7, epoch))
    assert ld.data.data_ptr() == ptr and torch.equal(ld.source, data)
    assert not torch.equal(epochs[0][0][0], epochs[1][0][0])  # two epochs: different crops of the same images
    _, _, plain = _loader()
    for (x, y), (_, y0) in zip(epochs[0], list(plain)):
        assert torch.equal(y, y0)  # labels unchanged
    _, _, twin = _loader(augment=AugmentConfig(seed=7))
    twin.set_epoch(2)
    for (x, y), (x2, y2) in zip(epochs[1], list(twin)):
        assert torch.equal(x, x2) and torch.equal(y, y2)  # same (seed, epoch): same batches, whatever the instance
    _, _, other = _loader(augment=AugmentConfig(seed=8))
    other.set_epoch(2)
    assert not torch.equal(next(iter(other))[0], epochs[1][0][0])


def test_random_sampler_takes_one_permutation_per_epoch():
    data, labels, ld = _loader(sampler="random", seed=5, augment=AugmentConfig())
    _, _, plain = _loader(sampler="random", seed=5)
    ld.set_epoch(1)
    plain.set_epoch(1)
    for (x, y), (_, y0) in zip(list(ld), list(plain)):
        assert torch.equal(y, y0)  # the same stream of permutations with and without augmentation
    assert torch.equal(ld.data, augment_reference(data, None, 0, 1))  # a permutation: every row rewritten


def test_world_size_independence():
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    data, labels = synthetic_cifar(101, seed=1)
    cfg = AugmentConfig(pad=4, flip=True, seed=11)
    one = DeviceLoader(data, labels, batch_size=8, world_size=1, rank=0, device=CPU, augment=cfg)
    ranks = [DeviceLoader(data, labels, batch_size=8, world_size=2, rank=r, device=CPU, augment=cfg) for r in (0, 1)]
    for ld in [one] + ranks:
        ld.set_epoch(3)
        ld.data.fill_(0xA5)
        list(ld)
    assert torch.equal(one.data, augment_reference(data, None, 11, 3))
    for ld in ranks:
        mine = np.unique(ld.indices())
        rest = np.setdiff1d(np.arange(101), mine)
        assert torch.equal(ld.data[mine], one.data[mine])
        assert bool((ld.data[rest] == 0xA5).all())
    assert len(np.union1d(ranks[0].indices(), ranks[1].indices())) == 101


# ---- CLI ----------------------------------------------------------------------------------------------------------
def _parse(argv, batch_default=32):
    from distributeddataparallel_cifar10_amd.train import add_cli_args, config_from_args
    return config_from_args(add_cli_args(argparse.ArgumentParser(), batch_default=batch_default).parse_args(argv),
                            "data/CIFAR-10/")


def test_cli_flags():
    from distributeddataparallel_cifar10_amd.train import augment_config, make_train_loader
    off = _parse([])
    assert (off.augment, off.augment_pad, off.augment_flip) == (False, 4, True) and augment_config(off) is None
    on = _parse(["--augment", "--augment-pad", "2", "--augment-no-flip", "--seed", "5"])
    assert augment_config(on) == AugmentConfig(pad=2, flip=False, seed=5)
    assert augment_config(_parse(["--augment-pad", "2"])) is None  # the pad alone turns nothing on
    with pytest.raises(SystemExit):
        augment_config(_parse(["--augment", "--augment-pad", "9"]))
    with pytest.raises(SystemExit, match="3x32x32"):  # data of another shape: a clear message at start-up
        make_train_loader(_parse(["--augment"]), torch.zeros(4, 3, 64, 64, dtype=torch.uint8), torch.zeros(4),
                          batch_size=2, device=CPU)


def _main_no_ddp(tmp_path, monkeypatch, name, extra):
    import main_no_ddp as M
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    mj = tmp_path / f"{name}.json"
    cfg = _parse(["--synthetic", "256", "--epochs", "2", "--max-steps", "4", "--engine", "torch", "--metrics-json",
                  str(mj)] + extra, batch_default=64)
    cfg.checkpoint = False
    monkeypatch.setattr(M, "_cfg", cfg)
    monkeypatch.setattr(M, "device", CPU)
    torch.manual_seed(11)
    M.training_loop(NetResDeep(), M.prepare())
    return [r for r in map(json.loads, mj.read_text().splitlines()) if "epoch" in r]


def test_main_no_ddp_cpu_with_augment(tmp_path, monkeypatch):
    """main_no_ddp.py --synthetic 256 --epochs 2 --max-steps 4 --engine torch [--augment] on the CPU."""
    plain = _main_no_ddp(tmp_path, monkeypatch, "plain", [])
    aug = _main_no_ddp(tmp_path, monkeypatch, "aug", ["--augment"])
    assert [r["augment"] for r in plain] == [None, None]
    assert [r["augment"] for r in aug] == [{"pad": 4, "flip": True, "seed": 0}] * 2
    assert [r["steps"] for r in aug] == [4, 4]
    assert all(np.isfinite(r["loss"]) for r in aug)
    assert aug[0]["loss"] != plain[0]["loss"] and aug[1]["loss"] != plain[1]["loss"]


def _main_cpu_run(tmp_path, name, **kw):
    """main.py's per-rank flow (world size 1, CPU: FlatBucketDDP) with --augment; the epoch records."""
    from distributeddataparallel_cifar10_amd.train import (TrainConfig, build_model_for_rank, load_dataset,
                                                           make_train_loader, train_loop)
    mj = tmp_path / f"{name}.json"
    cfg = TrainConfig(synthetic=256, max_steps=4, engine="torch", augment=True, seed=2, metrics_json=str(mj), **kw)
    data, labels = load_dataset(cfg)
    loader = make_train_loader(cfg, data, labels, batch_size=cfg.batch_size, world_size=1, rank=0, device=CPU,
                               sampler="distributed", seed=0)
    torch.manual_seed(5)
    model = build_model_for_rank(cfg, 0, 1, CPU, data, labels, loader)
    train_loop(model, loader, 0, cfg)
    return [r for r in map(json.loads, mj.read_text().splitlines()) if "epoch" in r]


def test_resume_redraws_the_second_epoch(tmp_path):
    """One epoch + --resume into the second gives the second epoch's loss of the 2-epoch run bitwise: the draws depend
    on (seed, epoch, id) alone, nothing of them is in the checkpoint."""
    ck = str(tmp_path / "ck" / "birds_vs_airplanes.pt")
    straight = _main_cpu_run(tmp_path, "straight", epochs=2, checkpoint=False)
    _main_cpu_run(tmp_path, "first", epochs=1, checkpoint_path=ck)
    resumed = _main_cpu_run(tmp_path, "resumed", epochs=2, resume=ck, checkpoint=False)
    assert [r["epoch"] for r in straight] == [1, 2] and [r["epoch"] for r in resumed] == [2]
    assert resumed[0]["loss"] == straight[1]["loss"] and resumed[0]["augment"] == straight[1]["augment"]
    assert straight[0]["loss"] != straight[1]["loss"]
