"""ROI-align: the float64 reference of tests/test_ops_roi_gpu.py (a four-tap gather written from the definition; its
backward is its own autograd), held to ``ResNet101ROI.roi_align``."""
import pytest
import torch

from distributeddataparallel_cifar10_amd.apps import ppe

F64 = torch.float64


def roi_taps(lo, hi, k, s, dim):
    """Per box and bin along one axis: (first tap, second tap, weight of the second tap, clamped coordinate)."""
    xs = lo[:, None] + (hi - lo)[:, None] * ((torch.arange(k, dtype=lo.dtype) + 0.5) / k)
    ix = (xs / s - 0.5).clamp(0, dim - 1)
    i0 = ix.floor()
    return i0.long(), (i0.long() + 1).clamp(max=dim - 1), ix - i0, ix


def roi_ref(feat, boxes, k, s):
    """feat [B, h, w, C], boxes [N, 5] (both float64) -> [N, k, k, C]."""
    _, h, w, _ = feat.shape
    x0, x1, fx, _ = roi_taps(boxes[:, 1], boxes[:, 3], k, s, w)
    y0, y1, fy, _ = roi_taps(boxes[:, 2], boxes[:, 4], k, s, h)
    b, wy, wx = boxes[:, 0].long()[:, None, None], fy[:, :, None, None], fx[:, None, :, None]
    tap = lambda y, x: feat[b, y[:, :, None], x[:, None, :]]  # noqa: E731
    return ((1 - wy) * (1 - wx) * tap(y0, x0) + (1 - wy) * wx * tap(y0, x1)
            + wy * (1 - wx) * tap(y1, x0) + wy * wx * tap(y1, x1))


def dyadic_boxes(h, w):
    """B = 3, stride 16: x1, y1 even, sides multiples of 16 (plus the dataset's dummy box); batch indices out of order,
    image 1 without a box, overhangs on all four borders, boxes 1 and 4 overlapping on image 0."""
    W, H = 16.0 * w, 16.0 * h
    return torch.tensor([[2, 0, 0, 10, 10], [0, 16, 32, 80, 96], [2, -16, -32, 48, 32],
                         [0, W - 32, H - 32, W + 16, H + 16], [0, 18, 34, 66, 98]], dtype=F64)


def random_boxes(n, B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=F64)  # noqa: E731
    x1, y1 = r(0, 16 * w - 64), r(0, 16 * h - 64)
    return torch.stack([torch.randint(0, B, (n,), generator=g).to(F64), x1, y1, x1 + r(16, 64), y1 + r(16, 64)], 1)


@pytest.mark.parametrize("h,w", [(8, 10), (5, 7)])
@pytest.mark.parametrize("k", [2, 4])
def test_reference(h, w, k):
    """It is the model's roi_align (random boxes, all four borders), and on the dyadic boxes every coordinate and
    weight is a multiple of 1/64: "exact" in the GPU tests means something."""
    feat = torch.randn(3, h, w, 6, generator=torch.Generator().manual_seed(0), dtype=F64)
    border = torch.tensor([[1, -40, -40, 30, 30], [2, 16 * w - 30, 16 * h - 30, 16 * w + 40, 16 * h + 40]], dtype=F64)
    boxes = torch.cat([random_boxes(6, 3, h, w, 1), border, dyadic_boxes(h, w)])
    got = roi_ref(feat, boxes, k, 16.0)
    want = ppe.ResNet101ROI(3, bins=k, layers=(1, 1, 1, 1)).roi_align(feat.permute(0, 3, 1, 2), boxes, 16.0)
    assert (got - want.permute(0, 2, 3, 1)).abs().max() <= 1e-12
    boxes = dyadic_boxes(h, w)
    for lo, hi, dim in ((boxes[:, 1], boxes[:, 3], w), (boxes[:, 2], boxes[:, 4], h)):
        for v in roi_taps(lo, hi, k, 16.0, dim)[2:]:
            assert torch.equal(v * 64, (v * 64).round())
