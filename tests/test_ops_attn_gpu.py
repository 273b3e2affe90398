"""Fused attention kernels (csrc/ops_attn.hip) on the GPU against float64, ``ops.attention`` through autograd, a
VisionTransformer step under OpsModel and the CLI."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from test_ops_attn import BF16, CASES, GAINS, attn_case, attn_errors, rel

pytestmark = pytest.mark.gpu
SCALE = 64 ** -0.5


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("b,h,l", CASES)
def test_kernels_against_float64(gpu, b, h, l, gain):
    """o, dq, dk, dv: every element written and finite, two launches bitwise equal, and a relative L2 error against
    float64 of at most twice that of torch's CPU scaled_dot_product_attention on the same bf16 tensors, plus 2^-8 (one
    bf16 rounding of the stored result, 2^-9 per element, doubled).  ``attn_errors`` says what the error of an exactly
    zero gradient (dq, dk of a single key) is measured against."""
    from distributeddataparallel_cifar10_amd.ops import functional as F
    case = attn_case(b, h, l, gain)
    qkv, dout = case["qkv"].to(gpu), case["dout"].to(gpu)
    runs = []
    for _ in range(2):
        o, lse = F.attention_fwd(qkv, SCALE)
        N = F.N
        o.fill_(float("nan")), lse.fill_(float("nan"))
        N.check(N.lib().dca_ops_attn_fwd(N.ptr(qkv), N.ptr(o), N.ptr(lse), b, l, h, 64, SCALE, N.stream(gpu)), "fwd")
        dqkv = torch.full_like(qkv, float("nan"))
        N.check(N.lib().dca_ops_attn_bwd(N.ptr(qkv), N.ptr(o), N.ptr(lse), N.ptr(dout), N.ptr(dqkv), b, l, h, 64,
                                         SCALE, N.stream(gpu)), "bwd")
        runs.append((o.cpu(), lse.cpu(), dqkv.cpu()))
    (o, lse, dqkv), again = runs
    assert all(torch.isfinite(t).all() for t in (o, lse, dqkv))
    assert all(torch.equal(x, y) for x, y in zip(runs[0], again))
    q, k = (case["qkv"][:, :, s].double().transpose(1, 2) for s in (0, 1))
    # lse is fp32 arithmetic throughout; 64 x 2^-24 is the worst-case bound of its 64-term dot products alone
    assert rel(lse, torch.logsumexp(q @ k.transpose(-1, -2) * SCALE, -1)) <= 2 ** -18
    errs = attn_errors(o, dqkv, case)
    print("attn", (b, h, l, gain), "errors", errs, "yardstick", case["yard"])
    assert all(e <= 2.0 * y + 2 ** -8 for e, y in zip(errs, case["yard"])), (errs, case["yard"])


def test_public_function(gpu):
    from distributeddataparallel_cifar10_amd.ops import attention
    from distributeddataparallel_cifar10_amd.ops import functional as F
    g = torch.Generator().manual_seed(65)
    qkv = torch.randn(2, 65, 3, 3, 64, generator=g).to(BF16).to(gpu)  # (B, H, L) = (2, 3, 65)
    dout = torch.randn(2, 65, 3, 64, generator=g).to(BF16).to(gpu)
    x = qkv.view(2, 65, 576).clone().requires_grad_()
    out = attention(x, 3)
    assert out.shape == (2, 65, 192) and out.dtype == BF16
    out.backward(dout.view(2, 65, 192))
    o, lse = F.attention_fwd(qkv, SCALE)
    assert torch.equal(out.detach().view_as(o), o)
    assert torch.equal(x.grad.view_as(qkv), F.attention_bwd(qkv, o, lse, dout, SCALE))
    with torch.no_grad():
        quiet = attention(qkv, 3)  # the 5-d form
    assert torch.equal(quiet.view_as(o), o) and quiet.grad_fn is None  # (no graph: nothing is saved)
    with pytest.raises(ValueError, match="contiguous"):
        attention(qkv.view(2, 65, 576).transpose(0, 1)[:, :2], 3)
    with pytest.raises(ValueError, match="heads"):
        attention(qkv.view(2, 65, 576), 5)
    with pytest.raises(ValueError, match="D == 64"):
        attention(qkv.view(2, 65, 576), 2)  # 3 * 2 * 96
    with pytest.raises(ValueError, match="1 <= L <= 256"):
        attention(torch.zeros(1, 257, 192, dtype=BF16, device=gpu), 1)


def test_vit_step_and_eval(gpu):
    """A two-block VisionTransformer (L = 17) trains one step under OpsModel: loss and every parameter gradient against
    the fp32 module on the CPU with the metric, k and c of tests/test_ops_gconv_gpu.py::test_resnext_step_and_eval
    (within 2x of stock bf16 autocast's own error on that step, + 0.02); then an eval-mode forward."""
    from distributeddataparallel_cifar10_amd.models.vit import VisionTransformer
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    with torch.random.fork_rng(devices=[gpu]):
        torch.manual_seed(0)
        ref = VisionTransformer(img_size=32, patch=8, dim=128, depth=2, heads=2, num_classes=10)
        x, y = torch.randn(2, 3, 32, 32), torch.randint(0, 10, (2,))
    amp, net = copy.deepcopy(ref), copy.deepcopy(ref).to(gpu)
    model = OpsModel(net)
    loss = cross_entropy(model(x.to(gpu)), y.to(gpu))
    loss.backward()
    lref = TF.cross_entropy(ref(x), y)
    lref.backward()
    with torch.autocast("cpu", dtype=BF16):
        lamp = TF.cross_entropy(amp(x), y)
    lamp.backward()
    k, c = 2.0, 0.02
    assert abs(loss.item() - lref.item()) <= k * abs(lamp.item() - lref.item()) + c * max(1.0, lref.item())
    rows = [(n, rel(p.grad, q.grad), rel(r.grad, q.grad)) for (n, p), (_, q), (_, r) in
            zip(net.named_parameters(), ref.named_parameters(), amp.named_parameters())]
    print("vit step", loss.item(), lref.item(), lamp.item(), rows)
    bad = [(n, e, a) for n, e, a in rows if e > k * a + c]
    assert not bad, bad
    model.eval(), ref.eval(), amp.eval()
    with torch.no_grad():
        out, want = model(x.to(gpu)), ref(x)
        with torch.autocast("cpu", dtype=BF16):
            aout = amp(x)
    assert rel(out, want) <= k * rel(aout.float(), want) + c


def test_main_no_ddp_vit(gpu):
    """main_no_ddp.py --engine ops --model vit trains a step (ViT-Tiny on the CIFAR tensors, L = 65)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "main_no_ddp.py", "--synthetic", "128", "--epochs", "1", "--max-steps", "1",
                        "--engine", "ops", "--model", "vit"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Epoch 1, Training loss" in r.stdout and "training time:" in r.stdout
