"""``ops.roi_align`` (csrc/ops_roi.hip) on an MI355X against the float64 reference of tests/test_ops_roi.py: bit for
bit where every product and sum is exact in fp32, general and hostile boxes, and reached from ``ResNet101ROI``."""
import copy

import pytest
import torch

from test_ops_roi import dyadic_boxes, random_boxes, roi_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
B = 3


def _ref(feat, boxes, k, dout):  # (out, dfeat) of the float64 reference, on the CPU
    f = feat.detach().double().cpu().requires_grad_()
    out = roi_ref(f, boxes.double().cpu(), k, 16.0)
    out.backward(dout.double().cpu())
    return out.detach(), f.grad


@pytest.mark.parametrize("h,w", [(8, 10), (5, 7)])
@pytest.mark.parametrize("C", [8, 72, 1024])
@pytest.mark.parametrize("k", [2, 4])
def test_exact(gpu, k, C, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N, roi_align
    boxes, g = dyadic_boxes(h, w), torch.Generator().manual_seed(0)
    feat = torch.randint(-8, 9, (B, h, w, C), generator=g).to(BF16).to(gpu)  # integers: exact in bf16
    dout = torch.randint(-3, 4, (len(boxes), k, k, C), generator=g).to(BF16).to(gpu)
    want, dwant = _ref(feat, boxes, k, dout)
    dboxes = boxes.float().to(gpu)
    got = roi_align(feat, dboxes, k, 16.0)
    assert got.dtype == BF16 and torch.equal(got.cpu(), want.to(BF16))
    dfeat = torch.full((B, h, w, C), float("nan"), dtype=BF16, device=gpu)  # an unwritten pixel shows
    N.check(N.lib().dca_ops_roi_align_bwd(N.ptr(dout), N.ptr(dboxes), N.ptr(dfeat), B, h, w, C, len(boxes), k, 16.0,
                                          N.stream(gpu)), "roi_align_bwd")
    assert torch.equal(dfeat.cpu(), dwant.to(BF16)) and not dfeat[1].any()


@pytest.mark.parametrize("k,C,h,w", [(4, 1024, 8, 10), (3, 72, 5, 7), (8, 8, 64, 33)])
def test_general_boxes(gpu, k, C, h, w):
    """|got - ref| <= 2^-8 |ref| + 1e-5 max|input|: one bf16 rounding at half an ulp, doubled, plus the fp32 coordinate
    error (a few ulp at magnitude <= 64) times the largest tap difference.  (64, 33): several pixel tiles backward."""
    from distributeddataparallel_cifar10_amd.ops import roi_align
    g = torch.Generator().manual_seed(2)
    boxes = random_boxes(7, B, h, w, 3).float()
    feat = torch.randn(B, h, w, C, generator=g).to(BF16).to(gpu).requires_grad_()
    dout = torch.randn(7, k, k, C, generator=g).to(BF16).to(gpu)
    roi_align(feat, boxes.to(gpu), k, 16.0).backward(dout)
    got = roi_align(feat, boxes.to(gpu), k, 16.0)
    for name, a, ref, src in zip(("out", "dfeat"), (got, feat.grad), _ref(feat, boxes, k, dout), (feat, dout)):
        err = (a.detach().double().cpu() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * src.detach().abs().max().item()
        assert (err <= bound).all(), name


def test_hostile_boxes(gpu):
    """A batch index of -1, one of B, NaN coordinates: exactly what the clamps make of them (image 0, image B - 1, the
    sample at pixel (0, 0)) both ways, finite, and no other row moves."""
    from distributeddataparallel_cifar10_amd.ops import roi_align
    bad = random_boxes(6, B, 8, 10, 4).float()
    clamped = bad.clone()
    bad[1, 0], bad[3, 0], bad[4, 1:] = -1.0, float(B), float("nan")
    clamped[1, 0], clamped[3, 0], clamped[4, 1:] = 0.0, B - 1.0, -1e4
    feat = torch.randn(B, 8, 10, 72, generator=torch.Generator().manual_seed(5)).to(BF16).to(gpu).requires_grad_()
    outs = [roi_align(feat, t.to(gpu), 4, 16.0) for t in (bad, clamped)]
    grads = [torch.autograd.grad(o, feat, o.detach())[0] for o in outs]
    assert outs[0].isfinite().all() and torch.equal(*outs) and grads[0].isfinite().all() and torch.equal(*grads)


def test_reached_from_the_model(gpu, monkeypatch):
    """No grid_sample in the default ops path, and a PPE step that repeats bit for bit."""
    from distributeddataparallel_cifar10_amd.apps import ppe
    monkeypatch.setattr(torch.nn.functional, "grid_sample", None)  # calling it raises a TypeError
    torch.manual_seed(0)
    ds = ppe.SyntheticPPE(2, seed=0)
    imgs, boxes, labels, _ = ds.detection_collate([ds[0], ds[1]])
    x, boxes, labels = ppe.preprocess_img(imgs.to(gpu).float()), boxes.to(gpu), labels.to(gpu)
    models = [ppe.build_model(None, 3, layers=(1, 1, 1, 1)).to(gpu)]
    models.append(copy.deepcopy(models[0]))
    for m in models:
        torch.nn.functional.binary_cross_entropy_with_logits(m(x, boxes), labels).backward()
    for (n, p), q in zip(models[0].named_parameters(), models[1].parameters()):
        assert p.grad is not None and p.grad.isfinite().all(), n
        if n.startswith(("stem", "layer1", "layer2", "layer3")):
            assert torch.equal(p.grad, q.grad), n
    monkeypatch.setattr(ppe, "OPS_ROI", False)  # DCA_OPS_ROI=0
    with pytest.raises(TypeError, match="not callable"):
        models[0](x, boxes)
