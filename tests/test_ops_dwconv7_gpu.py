"""The depthwise 7x7 kernels (csrc/ops_dwconv7.hip) on an MI355X against torch's float64 conv2d(groups=C)
(tests/test_ops_dwconv7.py): integer inputs make every fp32 sum and every bf16 output exact, so forward, input gradient,
weight gradient and bias gradient are compared bit for bit.  Then ``ops.conv2d`` through autograd, a ConvNeXt step under
OpsModel and the CLI."""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from test_ops_dwconv7 import dwconv7_case

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# (C, N, H, W): only the centre tap inside the image; an image smaller than the kernel's reach; two groups of rows; the
# widest row, five 8-channel slabs; the ring wraps, several strips, odd width; a ragged last slab of the 16-column form
SHAPES = [(8, 1, 1, 1), (8, 2, 3, 3), (24, 1, 7, 7), (40, 1, 9, 64), (16, 1, 20, 63), (136, 2, 5, 13)]


@functools.lru_cache(maxsize=None)
def _case(c, n, h, w):  # inputs and float64 reference, computed once per case and never modified
    return dwconv7_case(c, n, h, w)


@pytest.mark.parametrize("c,n,h,w", SHAPES)
def test_kernels_against_float64(gpu, c, n, h, w):
    from distributeddataparallel_cifar10_amd.ops import _native as N
    from distributeddataparallel_cifar10_amd.ops import functional as F
    x, wt, b, dy, y_ref, dx_ref, dw_ref, db_ref = _case(c, n, h, w)
    xd, dyd, wd, bd = x.to(BF16).to(gpu), dy.to(BF16).to(gpu), wt.float().to(gpu), b.float().to(gpu)
    dw0 = torch.arange(dw_ref.numel(), dtype=torch.float32).view(dw_ref.shape) % 17 - 8  # a gradient already there
    db0 = torch.arange(c, dtype=torch.float32) % 5 - 2
    runs = []
    for _ in range(2):
        outs = []
        for src, bias, flip in ((xd, bd, 0), (xd, None, 0), (dyd, None, 1)):  # y with and without bias, dx
            out = torch.full(y_ref.shape, float("nan"), dtype=BF16, device=gpu)
            N.check(N.lib().dca_ops_dwconv7_fwd(N.ptr(src), N.ptr(wd), N.ptr(bias), N.ptr(out), n, h, w, c, flip,
                                                N.stream(gpu)), "dwconv7_fwd")
            outs.append(out.cpu())
        for slabs in (1, 3):
            dw, db = F.dwconv7_wgrad(xd, dyd, slabs=slabs)
            sink = (dw0.to(gpu), db0.to(gpu))
            F.dwconv7_wgrad(xd, dyd, out=sink, slabs=slabs)  # beta = 1
            outs += [dw.cpu(), db.cpu(), sink[0].cpu(), sink[1].cpu()]
        runs.append(outs)
    assert all(torch.equal(p, q) for p, q in zip(*runs))  # (NaN, an unwritten element, is unequal to itself)
    y, y_nobias, dx = runs[0][:3]
    assert torch.equal(y.double(), y_ref) and torch.equal(y_nobias.double(), y_ref - b) and torch.equal(dx.double(), dx_ref)
    for dw, db, sdw, sdb in (runs[0][3:7], runs[0][7:11]):
        assert torch.equal(dw.double(), dw_ref) and torch.equal(db.double(), db_ref)
        assert torch.equal(sdw.double(), dw0.double() + dw_ref) and torch.equal(sdb.double(), db0.double() + db_ref)


def test_conv2d_through_autograd(gpu):
    from distributeddataparallel_cifar10_amd.ops import conv2d
    from distributeddataparallel_cifar10_amd.ops import functional as F
    x, wt, b, dy = (t.to(gpu) for t in _case(40, 1, 9, 64)[:4])
    xd, dyd = x.to(BF16).requires_grad_(), dy.to(BF16)
    wd, bd = wt.float().requires_grad_(), b.float().requires_grad_()
    y = conv2d(xd, wd, bd, stride=1, pad=3, groups=40)
    y.backward(dyd)
    assert torch.equal(y.detach(), F.dwconv7_fwd(xd.detach(), wd.detach(), bd.detach()))
    assert torch.equal(xd.grad, F.dwconv7_dgrad(dyd, wd.detach()))
    dw, db = F.dwconv7_wgrad(xd.detach(), dyd)
    assert torch.equal(wd.grad, dw) and torch.equal(bd.grad, db)


def _rel(a, b):  # tests/test_ops_gpu.py:13
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_convnext_step_and_eval(gpu):
    """A two-stage ConvNeXt (8 x 8 and 4 x 4 grids) trains one step under OpsModel: loss and every parameter gradient
    against the fp32 module on the CPU with the metric, k and c of tests/test_ops_attn_gpu.py::test_vit_step_and_eval
    (within 2x of stock bf16 autocast's own error on that step, + 0.02); then an eval-mode forward."""
    from distributeddataparallel_cifar10_amd.models.convnext import ConvNeXt
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    with torch.random.fork_rng(devices=[gpu]):
        torch.manual_seed(0)
        ref = ConvNeXt(depths=(1, 1), dims=(64, 128), num_classes=10, layer_scale=1.0)
        x, y = torch.randn(2, 3, 32, 32), torch.randint(0, 10, (2,))
    amp, net = copy.deepcopy(ref), copy.deepcopy(ref).to(gpu)
    model = OpsModel(net)
    assert model.kind == "convnext"
    loss = cross_entropy(model(x.to(gpu)), y.to(gpu))
    loss.backward()
    lref = TF.cross_entropy(ref(x), y)
    lref.backward()
    with torch.autocast("cpu", dtype=BF16):
        lamp = TF.cross_entropy(amp(x), y)
    lamp.backward()
    k, c = 2.0, 0.02
    rows = [(n, _rel(p.grad, q.grad), _rel(r.grad, q.grad)) for (n, p), (_, q), (_, r) in
            zip(net.named_parameters(), ref.named_parameters(), amp.named_parameters())]
    print("convnext step", loss.item(), lref.item(), lamp.item(), rows)
    assert abs(loss.item() - lref.item()) <= k * abs(lamp.item() - lref.item()) + c * max(1.0, lref.item())
    bad = [(n, e, a) for n, e, a in rows if e > k * a + c]
    assert not bad, bad
    model.eval(), ref.eval(), amp.eval()
    with torch.no_grad():
        out, want = model(x.to(gpu)), ref(x)
        with torch.autocast("cpu", dtype=BF16):
            aout = amp(x)
    assert _rel(out, want) <= k * _rel(aout.float(), want) + c


def test_main_no_ddp_convnext(gpu):
    """main_no_ddp.py --engine ops --model convnext trains a step (ConvNeXt-T on the CIFAR tensors: grids 8 / 4 / 2 / 1)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "main_no_ddp.py", "--synthetic", "128", "--epochs", "1", "--max-steps", "1",
                        "--engine", "ops", "--model", "convnext"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Epoch 1, Training loss" in r.stdout and "training time:" in r.stdout
