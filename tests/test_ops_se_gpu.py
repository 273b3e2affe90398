"""The squeeze-and-excitation kernels (csrc/ops_se.hip) on an MI355X against float64 (tests/test_ops_se.py): bit for bit
on inputs that make every value exact, within the kernels' own roundings on real-valued ones, and through autograd."""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from test_ops_se import se_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# (N, H, W, C).  The slab is 8 chunks (32 pixel lanes), 16 (16 lanes) when P <= 256 and C >= 128, 32 (8 lanes) when
# P <= 64 and C >= 256; the walk is unrolled by four pixels per lane.
SHAPES = [(1, 1, 1, 8),       # one chunk and one pixel
          (2, 2, 2, 16),      # two images, P = 4 below the 32 lanes
          (1, 5, 13, 40),     # 8-chunk slab, ragged (5 chunks); P = 65 = 2 x 32 + 1
          (1, 10, 13, 72),    # 8-chunk slabs, the second ragged; P = 130: the unrolled walk and its tail
          (2, 7, 7, 136),     # 16-chunk slabs, the second ragged (1 chunk); P = 49 = 3 x 16 + 1
          (1, 16, 16, 128),   # 16-chunk slab at its largest P; 16 pixels per lane
          (1, 257, 1, 128),   # one pixel more: back to 8-chunk slabs
          (1, 8, 8, 256),     # 32-chunk slab at its largest P
          (1, 5, 13, 264),    # one pixel more: 16-chunk slabs, three, the last ragged
          (1, 5, 7, 264)]     # 32-chunk slabs, the second ragged (1 chunk); P = 35 = 4 x 8 + 3


@functools.lru_cache(maxsize=None)
def _inputs(shape, exact):  # (u, z, idt, dout, ds) on the CPU, computed once per case and never modified
    n, h, w, c = shape
    g = torch.Generator().manual_seed(sum(shape) + exact)
    if exact:  # g = sigmoid(z) is exactly 1/2 or 1 in fp32; ds / P is an integer
        u, idt, dout = (torch.randint(-4, 5, shape, generator=g).to(BF16) for _ in range(3))
        z = 64.0 * torch.randint(0, 2, (n, c), generator=g)
        ds = float(h * w) * torch.randint(-4, 5, (n, c), generator=g)
    else:
        u, idt, dout = (torch.randn(shape, generator=g).to(BF16) for _ in range(3))
        z = 2.0 * torch.randn(n, c, generator=g)
        ds = torch.randn(n, c, generator=g).to(BF16)
    return u, z, idt, dout, ds


def _kernels(gpu, shape, exact, s_dtype):
    from distributeddataparallel_cifar10_amd.ops import functional as F
    u, z, idt, dout, ds = (t.to(gpu) for t in _inputs(shape, exact))
    s = F.se_squeeze_fwd(u, s_dtype)
    out = F.se_scale_fwd(u, z, idt)
    didt, dz = F.se_bwd_reduce(dout, out, u, z)
    du = F.se_bwd_apply(dout, out, z, ds)
    return [t.cpu() for t in (s, out, didt, dz, du)]


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_and_repeatable(gpu, shape):
    first, again = _kernels(gpu, shape, True, torch.float32), _kernels(gpu, shape, True, torch.float32)
    ref = se_ref(*_inputs(shape, True))
    for name, a, b, r in zip(("s", "out", "didt", "dz", "du"), first, again, ref):
        assert torch.equal(a, b), name
        assert torch.equal(a.double(), r.float().double() if name == "s" else r), name  # (s: one fp32 division)
    assert torch.equal(_kernels(gpu, shape, True, BF16)[0], ref[0].float().to(BF16))


@pytest.mark.parametrize("shape", SHAPES)
def test_real_valued(gpu, shape):
    u, z, idt, dout, ds = _inputs(shape, False)
    p = shape[1] * shape[2]
    (s, out, didt, dz, du), s16 = _kernels(gpu, shape, False, torch.float32), _kernels(gpu, shape, False, BF16)[0]
    s_ref, out_ref, _, _, _ = se_ref(u, z, idt, dout, ds)
    _, _, didt_ref, dz_ref, du_ref = se_ref(u, z, idt, dout, ds, out=out)  # the mask of the saved output
    # one bf16 rounding (half a spacing of 2^-7) with its boundary moved by the fp32 error, + fp32 cancellation near 0
    near0 = 2.0 ** -16 * (u.double().abs().max() + idt.double().abs().max())
    assert ((out.double() - out_ref).abs() <= 2.0 ** -8 * out_ref.abs() + near0).all()
    assert ((du.double() - du_ref).abs() <= 2.0 ** -8 * du_ref.abs() + near0).all()
    assert torch.equal(didt.double(), didt_ref)  # a select: no rounding
    s_tol = 2.0 ** -22 * u.double().abs().sum((1, 2)) / p
    assert ((s.double() - s_ref).abs() <= s_tol).all()
    assert ((s16.double() - s_ref).abs() <= s_tol + 2.0 ** -8 * s_ref.abs()).all()  # + its one bf16 rounding
    # a P-term fp32 sum, doubled (g (1 - g) <= 1 / 4 leaves room for the gate's own fp32 error)
    assert ((dz.double() - dz_ref).abs() <= p * 2.0 ** -23 * (dout.double() * u.double()).abs().sum((1, 2))).all()


def _rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _bf(m):  # a float64 CPU copy of a module with its weight rounded to bf16 (what the GEMMs read)
    r = copy.deepcopy(m).cpu().double()
    with torch.no_grad():
        r.weight.copy_(m.weight.detach().to(BF16).double())
    return r


@pytest.mark.parametrize("joined", [False, True])
def test_autograd_composite(gpu, joined):
    """se_squeeze -> linear + ReLU -> linear -> se_scale against the float64 composite, with the yardstick of
    test_conv_bn_act (2e-2 forward, 3e-2 gradients).  joined: u = bn(conv1x1(h)) and the identity is h itself, whose
    gradient is se_scale's contribution to a GradJoin plus the conv's input gradient accumulated into it.  The same
    forward under no_grad gives the same bits."""
    from distributeddataparallel_cifar10_amd.ops import SELink, conv_bn_act, linear, se_scale, se_squeeze
    from distributeddataparallel_cifar10_amd.ops.functional import GradJoin
    n, hw, c, r = 2, 6, 128, 16
    with torch.random.fork_rng(devices=[gpu]):
        torch.manual_seed(5 + joined)
        conv, bn = torch.nn.Conv2d(c, c, 1, bias=False).to(gpu), torch.nn.BatchNorm2d(c).to(gpu)
        fc1, fc2 = torch.nn.Linear(c, r).to(gpu), torch.nn.Linear(r, c).to(gpu)
        h = torch.randn(n, hw, hw, c, device=gpu).to(BF16).requires_grad_()
        other = torch.randn(n, hw, hw, c, device=gpu).to(BF16).requires_grad_()
        dy = torch.randn(n, hw, hw, c, device=gpu).to(BF16)
    rconv, rbn, rfc1, rfc2 = _bf(conv), copy.deepcopy(bn).cpu().double(), _bf(fc1), _bf(fc2)

    def forward():
        join = GradJoin(2) if joined and torch.is_grad_enabled() else None
        u = conv_bn_act(h, conv, bn, relu=False, x_join=join) if joined else h
        link = SELink()
        s = linear(se_squeeze(u, link), fc1.weight, fc1.bias, relu=True, out_dtype=BF16)
        z = linear(s, fc2.weight, fc2.bias, out_dtype=torch.float32)
        return se_scale(u, z, h if joined else other, link, x_join=join)

    out = forward()
    out.backward(dy)
    with torch.no_grad():
        assert torch.equal(forward(), out)
    hr, orr = h.detach().cpu().double().requires_grad_(), other.detach().cpu().double().requires_grad_()
    ur = rbn(rconv(hr.permute(0, 3, 1, 2))).permute(0, 2, 3, 1) if joined else hr
    zr = rfc2(torch.relu(rfc1(ur.mean((1, 2)))))
    ref = torch.relu(ur * torch.sigmoid(zr)[:, None, None, :] + (hr if joined else orr))
    ref.backward(dy.cpu().double())
    assert _rel(out, ref) < 2e-2
    pairs = [(h, hr), (fc1.weight, rfc1.weight), (fc1.bias, rfc1.bias), (fc2.weight, rfc2.weight), (fc2.bias, rfc2.bias)]
    pairs += [(conv.weight, rconv.weight), (bn.weight, rbn.weight)] if joined else [(other, orr)]
    bad = [(i, e) for i, e in enumerate(_rel(a.grad, b.grad) for a, b in pairs) if not e < 3e-2]
    assert not bad, bad


def test_se_resnet_step_and_eval(gpu):
    """test_ops_resnet_step's recipe on an SE net: loss and every parameter gradient within 2x of stock bf16 autocast's
    own error against fp32, + 0.02; every se.* parameter has a gradient; then an eval-mode forward under no_grad."""
    from distributeddataparallel_cifar10_amd.models.resnet50 import ResNet
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    with torch.random.fork_rng(devices=[gpu]):
        torch.manual_seed(0)
        net = ResNet([1, 1, 1, 1], num_classes=10, zero_init_residual=False, se_reduction=16).to(gpu)
        x, y = torch.randn(8, 3, 128, 128, device=gpu), torch.randint(0, 10, (8,), device=gpu)
    ref, amp = copy.deepcopy(net), copy.deepcopy(net)
    model = OpsModel(net)
    loss = cross_entropy(model(x), y)
    loss.backward()
    lref = TF.cross_entropy(ref(x), y)
    lref.backward()
    with torch.autocast("cuda", dtype=BF16):
        lamp = TF.cross_entropy(amp(x), y)
    lamp.backward()
    k, c = 2.0, 0.02
    assert abs(loss.item() - lref.item()) <= k * abs(lamp.item() - lref.item()) + c * max(1.0, lref.item())
    names = [n for n, _ in net.named_parameters()]
    assert sum(".se." in n for n in names) == 16 and all(p.grad is not None for p in net.parameters())
    rows = [(n, _rel(p.grad, q.grad), _rel(r.grad, q.grad))
            for n, p, q, r in zip(names, net.parameters(), ref.parameters(), amp.parameters())]
    print("\n".join(f"{n:40s} ops {e:.4f}  autocast {a:.4f}" for n, e, a in rows))
    bad = [(n, e, a) for n, e, a in rows if not e <= k * a + c]
    assert not bad, bad
    model.eval(), ref.eval(), amp.eval()
    with torch.no_grad():
        out, want = model(x), ref(x)
        with torch.autocast("cuda", dtype=BF16):
            aout = amp(x)
    assert _rel(out, want) <= k * _rel(aout.float(), want) + c


def test_main_no_ddp_seresnext50(gpu):
    """main_no_ddp.py --engine ops --model seresnext50 trains a step (identity and downsample SE blocks)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "main_no_ddp.py", "--synthetic", "128", "--epochs", "1", "--max-steps", "1",
                        "--engine", "ops", "--model", "seresnext50"], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Epoch 1, Training loss" in r.stdout and "training time:" in r.stdout
