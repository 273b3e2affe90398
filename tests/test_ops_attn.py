"""Fused attention on the ops path (csrc/ops_attn.hip), the parts that need no GPU: the launchers' shape rule, the
argument checks of ``ops.attention``, the VisionTransformer, and the float64 reference and bf16 yardstick that
tests/test_ops_attn_gpu.py uses."""
import functools

import pytest
import torch
import torch.nn.functional as TF

BF16 = torch.bfloat16
CASES = [(1, 1, 1), (2, 3, 17), (1, 2, 65), (2, 3, 197), (1, 2, 256)]  # (B, H, L)
GAINS = [1.0, 8.0]  # q, k multiplied by this: at 8 the scaled scores reach several tens


def rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def attn_errors(o, dqkv, case):
    """Relative L2 errors of (o, dq, dk, dv) against the case's float64 values.  Where the float64 gradient is exactly
    zero (dq and dk of a single key: P = 1 and dS = P (dP - delta) = 0, while bf16 or fp32 arithmetic subtracts two
    sums of the same products taken in different orders) a relative error does not exist; the error is then measured
    against ``mag``, the gradient with its cancellations removed."""
    want = [case["o"]] + [case["dqkv"][:, :, s] for s in range(3)]
    den = [w.norm() if w.any() else case["mag"][:, :, i - 1].norm() for i, w in enumerate(want)]
    got = [o] + [dqkv[:, :, s] for s in range(3)]
    return [((g.double().cpu() - w).norm() / d).item() for g, w, d in zip(got, want, den)]


@functools.lru_cache(maxsize=None)
def attn_case(b, h, l, gain):
    """Seeded bf16 qkv [B, L, 3, H, 64] and dout [B, L, H, 64]; o and dqkv of the float64 composition on those rounded
    values; ``yard``: the errors (``attn_errors``) of torch's CPU ``scaled_dot_product_attention`` on the same bf16
    tensors."""
    g = torch.Generator().manual_seed(1000 * l + 10 * h + b)
    qkv = torch.randn(b, l, 3, h, 64, generator=g)
    qkv[:, :, :2] *= gain
    qkv, dout = qkv.to(BF16), torch.randn(b, l, h, 64, generator=g).to(BF16)
    x = qkv.double().requires_grad_()
    q, k, v = x.permute(2, 0, 3, 1, 4)  # each [B, H, L, D]
    p = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, -1)
    o = (p @ v).permute(0, 2, 1, 3)
    o.backward(dout.double())
    with torch.no_grad():  # sum_j P_ij (|dP_ij| + |delta_i|) |K_j| * scale, and the same for dk
        dp = dout.double().transpose(1, 2) @ v.transpose(-1, -2)
        a = p * (dp.abs() + (p * dp).sum(-1, keepdim=True).abs()) * 64 ** -0.5
        mag = torch.stack([a @ k.abs(), a.transpose(-1, -2) @ q.abs()]).permute(1, 3, 0, 2, 4)  # [B, L, 2, H, D]
    case = {"qkv": qkv, "dout": dout, "o": o.detach(), "dqkv": x.grad, "mag": mag}
    y = qkv.clone().requires_grad_()
    yq, yk, yv = y.permute(2, 0, 3, 1, 4)
    yo = TF.scaled_dot_product_attention(yq, yk, yv).permute(0, 2, 1, 3)
    yo.backward(dout)
    case["yard"] = attn_errors(yo.detach(), y.grad, case)
    return case


@pytest.mark.parametrize("shape,ok", [((2, 65, 3, 64), True), ((1, 1, 1, 64), True), ((1, 256, 12, 64), True),
                                      ((1, 0, 1, 64), False), ((1, 257, 1, 64), False), ((1, 1, 1, 32), False),
                                      ((1, 1, 1, 128), False), ((1, 1, 0, 64), False),
                                      ((1 << 14, 256, 8, 64), False),     # 3 * 2^29 elements
                                      ((1 << 13, 256, 5, 64), True)])     # 15 * 2^27 < 2^31
def test_rule_boundaries(shape, ok):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    assert (N.lib().dca_ops_attn_rule(*shape) == 0) == ok
    if not ok:
        assert b"attention rule is" in N.lib().dca_ops_last_error()


def test_argument_checks_and_fp8_refusal():
    from distributeddataparallel_cifar10_amd.models.vit import vit_tiny
    from distributeddataparallel_cifar10_amd.ops import OpsModel, attention
    with pytest.raises(ValueError, match="GPU tensors"):
        attention(torch.zeros(1, 4, 192, dtype=BF16), 1)
    with pytest.raises(TypeError, match="bfloat16"):
        attention(torch.zeros(1, 4, 192), 1)
    with torch.random.fork_rng(devices=[]):  # (the process's generator is left as it was found)
        net = vit_tiny(num_classes=10)
    with pytest.raises(ValueError, match="fp8 is not available for a vision transformer"):
        OpsModel(net, fp8=True)
    assert OpsModel(net).kind == "vit"


def test_vit_shape_and_split_order():
    """The module's attention equals softmax(q k^T * scale) v in float64 with q, k, v taken from the qkv linear's
    output viewed as [B, L, 3, H, D]: the split order the kernel assumes."""
    from distributeddataparallel_cifar10_amd.models.vit import VisionTransformer, vit_tiny
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        net = VisionTransformer(img_size=32, patch=8, dim=128, depth=1, heads=2, num_classes=10).double()
        tiny = vit_tiny(num_classes=10)
        x, img = torch.randn(2, 17, 128, dtype=torch.float64), torch.randn(2, 3, 32, 32)
    assert tiny(img).shape == (2, 10) and tiny.pos_embed.shape == (1, 65, 192)
    assert vit_tiny(img_size=224, patch=16).pos_embed.shape == (1, 197, 192)
    blk = net.blocks[0]
    qkv = blk.qkv(x).view(2, 17, 3, 2, 64)
    q, k, v = (qkv[:, :, s].transpose(1, 2) for s in range(3))  # [B, H, L, D]
    want = (torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, -1) @ v).transpose(1, 2).reshape(2, 17, 128)
    assert rel(blk.attention(x), want) < 1e-12


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("b,h,l", CASES)
def test_yardstick_is_usable(b, h, l, gain):
    """Stock bf16 attention's own error is finite for every case and non-zero wherever it can be: with a single key
    o = v and dv = dout without any rounding, and dq = dk = 0 in float64."""
    case = attn_case(b, h, l, gain)
    assert all(0.0 <= e < 2 ** -5 for e in case["yard"]), case["yard"]
    assert l == 1 or all(e > 0.0 for e in case["yard"]), case["yard"]
    assert l > 1 or not case["dqkv"][:, :, :2].any()
