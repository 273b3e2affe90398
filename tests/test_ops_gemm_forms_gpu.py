"""Every GEMM kernel instantiation dca_ops_gemm dispatches (csrc/ops_gemm_route.hip GEMM_KERNELS) in every epilogue
form its family's route admits, against float64, bit for bit.

The cases and forms are tests/_gemm_forms.py (tests/test_native_build.py::test_gemm_form_cases_cover_the_table proves
on the CPU that they cover the whole table).  Each call goes to dca_ops_gemm with the GemmArgs of
``_gemm_forms.gemm_fields`` and real buffers; afterwards dca_ops_gemm_last_route must name the kernel the case claims,
with the claimed splits / reduce / masked copy.

Why bitwise is the right comparison.  Operands are integers in [-3, 3] ({-1, 0, 1} under col_stats), exact in bf16
and fp8 e4m3; alpha is 1/2 (given as 0.5, or as 0.25 with alpha_dev = 2), the bias a multiple of 1/4 within +-2, beta
1 or -2, C_old an integer within +-8, the statistics shift a multiple of 1/2 within +-2.  Every accumulator is then an
integer and every value of  acc alpha + bias + beta C_old  a multiple of 1/4.  Each case asserts, on the float64
reference alone, that 4 |ref| < 2^24: all partial sums and products of the expression are then multiples of 1/4 below
2^22, exactly representable in fp32, so the fp32 result is float32(ref64) whatever the order of operations or FMA
contraction, and the bf16 output is that value rounded to nearest even (torch's conversion, as f2bf_rne and the
hardware convert).  Likewise the column statistics: d = stored output - shift is a multiple of 1/4 and d^2 of 1/16,
and each case asserts 4 sum|d| < 2^24 and 16 sum d^2 < 2^24 per column and 128-row partial row (over all rows for the
row-ring and direct kernels, whose partial rows are per workgroup: that bounds every partition); the float64 sum of
exact partial rows is then the exact total.  Comparisons are on integer bit patterns, so a NaN equals nothing but
itself.

Nothing else is written: the output is the view [:M, :N] of a parent [M + 1, ldc] pre-filled with a NaN bit pattern
(beta = 0) or with C_old in the view (beta != 0), and the whole parent is compared -- an unwritten element inside the
view, and a written one outside, both fail.  Row remaps (orow) keep the sentinel in the rows of the other parity
classes; a weight-layout remap (wperm) is compared over the whole [Cout, Cin, KH, KW] tensor plus a sentinel tail.
The split-K slab is pre-filled with NaN too.  The statistics buffer carries one sentinel row past the last partial
row; each 128-row partial row is compared exactly for gemm_epilogue, store_quarters_256 and the stream kernel (the
k_bn_finalize contract), the column totals for the row-ring and direct kernels (one row per workgroup).  A masked
accumulation source must leave its source and mask unchanged.

The one derived bound: the fp8 amax forms multiply by 1/448.f, which is not exact.  Counting the fp32 roundings of
gemm_alpha and the epilogue expression,  |err| <= 8 2^-24 (|acc alpha| + |bias| + |beta C_old|)  per element, plus
2^-8 |ref| (half a bf16 ulp) for a bf16 output; the largest error / bound ratio is printed (pytest -s).

(The module's name puts it after tests/test_ddp_engine_gpu.py and tests/test_multigpu.py in pytest's order, for the
reason tests/test_ops_bn_gpu.py gives.)"""
import ctypes
import math
import zlib

import pytest
import torch

import _gemm_forms as GF

pytestmark = pytest.mark.gpu

EXACT = float(1 << 24)
U32 = 2.0 ** -24
HALF = 2.0 ** -8
SENT32, SENT16 = 0x7FC12345, 0x7FC5   # NaN payloads
AMAX_A, AMAX_B = 3.0, 1.75
PTRS = ("A", "B", "C", "bias", "ws", "alpha_dev", "col_stats", "stats_shift", "amax_a", "amax_b", "beta_src",
        "beta_mask")


def _N():
    from distributeddataparallel_cifar10_amd.ops import _native
    return _native


def _report(what, err, bound):
    """Fails unless err <= bound everywhere (a NaN fails); prints the largest err / bound."""
    ok = err <= bound
    inf, zero = torch.full_like(err, math.inf), torch.zeros_like(err)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, zero, inf))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"ratio {what} {worst:.4f}")
    if not bool(ok.all()):
        i = int(torch.argmax(ratio.reshape(-1)))
        return (f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound; worst at flat index {i}: "
                f"error {err.reshape(-1)[i].item():.6g}, bound {bound.reshape(-1)[i].item():.6g}")
    return None


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sentinel(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    _bits(t).fill_(SENT32 if dtype == torch.float32 else SENT16)
    return t


def _im2col(x, kh, kw, s, p):
    """[n, h, w, c] float64 -> [n Ho Wo, kh kw c], column (tap, c)."""
    n, h, w, c = x.shape
    u = torch.nn.functional.unfold(x.permute(0, 3, 1, 2), (kh, kw), padding=p, stride=s)   # [n, c kh kw, L]
    return u.view(n, c, kh * kw, -1).permute(0, 3, 2, 1).reshape(-1, kh * kw * c)


class _Problem:
    """Operands of a case on the device (padding columns hold 7: reading them shows) and acc64 = A B^T."""

    def __init__(self, case, tern, dev):
        self.case, self.dev = case, dev
        self.gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) * 2 + int(tern))
        lo, hi = (-1, 2) if tern else (-3, 4)
        M, N, K = case.shape
        dt = torch.float8_e4m3fn if case.fp8 else torch.bfloat16

        def ints(*shape):
            return torch.randint(lo, hi, shape, generator=self.gen).float()

        def store(v, ld):   # [rows, cols] values into a [rows, ld] operand buffer
            buf = torch.full((v.shape[0], ld), 7.0)
            buf[:, :v.shape[1]] = v
            t = buf.to(dev).to(dt)
            return t.view(torch.uint8) if case.fp8 else t

        f = GF.gemm_fields(case, case.forms[0])
        if case.conv:
            n, h, w, c, co, kh, kw, s, p = case.geom
            x = ints(n, h, w, c)
            cols = _im2col(x.to(dev).double(), kh, kw, s, p)
            if case.conv == 1:
                wm = ints(N, K)
                self.A, self.B = x.to(dev).to(dt), store(wm, f["ldb"])
                self.acc = cols @ wm.to(dev).double().t()
            else:
                dy = ints(K, M)
                self.A, self.B = store(dy, f["lda"]), x.to(dev).to(dt)
                self.acc = dy.to(dev).double().t() @ cols
        else:
            a, b = ints(M, K), ints(N, K)
            self.A = store(a.t().contiguous() if case.ta else a, f["lda"])
            self.B = store(b.t().contiguous() if case.tb else b, f["ldb"])
            self.acc = a.to(dev).double() @ b.to(dev).double().t()
        assert self.acc.shape == (M, N)

    def ints(self, lo, hi, *shape, scale=1.0):
        return (torch.randint(lo, hi + 1, shape, generator=self.gen).float() * scale).to(self.dev)


def _run_form(prob, form, fails):
    N_ = _N()
    case, dev = prob.case, prob.dev
    tag = f"{case.id}/{form.name}"
    M, N, K = case.shape
    f = GF.gemm_fields(case, form)
    ldc = f["ldc"]
    dt = torch.float32 if form.out == "f32" else torch.bfloat16
    bufs = dict(A=prob.A, B=prob.B)

    # ---- epilogue constants and the float64 reference ----
    alpha64 = form.alpha * (form.alpha_dev if form.alpha_dev is not None else 1.0)
    if form.alpha_dev is not None:
        bufs["alpha_dev"] = torch.tensor([form.alpha_dev], dtype=torch.float32, device=dev)
    if form.amax:
        am = torch.tensor([AMAX_A, AMAX_B], dtype=torch.float32)
        bufs["amax_a"] = am[0:1].view(torch.int32).to(dev)
        bufs["amax_b"] = am[1:2].view(torch.int32).to(dev)
        alpha64 = alpha64 * (AMAX_A / 448.0) * (AMAX_B / 448.0)
    ref = prob.acc * alpha64
    mag = ref.abs()
    if form.bias:
        bufs["bias"] = prob.ints(-8, 8, N, scale=0.25)
        ref = ref + bufs["bias"].double()
        mag = mag + bufs["bias"].double().abs()
    if form.wperm is not None:   # GEMM column tap * Cpad + c -> [M, C, T], padded channels dropped
        C_, Cpad, T = form.wperm
        ref, mag = (v.view(M, T, Cpad)[:, :, :C_].permute(0, 2, 1) for v in (ref, mag))
    old = None
    if form.mask:
        assert ldc == N and N % 8 == 0
        src = prob.ints(-8, 8, M, N).to(torch.bfloat16)
        bits = torch.randint(0, 2, (M, N), generator=prob.gen).to(dev)
        wgt = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
        mask = (bits.view(-1, 8).to(torch.int32) * wgt).sum(1).to(torch.uint8).contiguous()
        bufs["beta_src"], bufs["beta_mask"] = src, mask
        src0, mask0 = src.clone(), mask.clone()
        old_term = form.beta * (src.double() * bits.double())
    elif form.beta != 0.0:
        old = prob.ints(-8, 8, *ref.shape).to(dt)
        old_term = form.beta * old.double()
    if form.beta != 0.0:
        ref = ref + old_term
        mag = mag + old_term.abs()
    if form.relu:
        ref = ref.clamp_min(0.0)
    if not form.amax:   # the exactness preconditions, on the reference alone
        assert float((ref * 4).abs().max()) < EXACT and bool(((ref * 4) == (ref * 4).round()).all()), tag

    # ---- the output parent: sentinel everywhere, C_old inside the view ----
    if form.wperm is not None:
        numel = M * C_ * T
        parent = _sentinel((numel + 16,), dt, dev)

        def view(t):
            return t[:numel].view(M, C_, T)
        if old is not None:
            view(parent).copy_(old)
        expected = parent.clone()
        view(expected).copy_(ref.float().to(dt))
    else:
        rows = M
        idx = torch.arange(M, device=dev)
        if form.orow:
            n, ho, wo, H, W, ph, pw = GF.orow_grid(M)
            j, t = idx % wo, idx // wo
            idx = ((t // ho) * H + 2 * (t % ho) + ph) * W + 2 * j + pw
            rows = n * H * W
        parent = _sentinel((rows + 1, ldc), dt, dev)
        if old is not None:
            parent[idx, :N] = old
        expected = parent.clone()
        expected[idx, :N] = ref.float().to(dt)
    bufs["C"] = parent
    if "ws" in f:
        bufs["ws"] = torch.full((case.splits * M * N,), float("nan"), dtype=torch.float32, device=dev)
    if form.stats:
        nparts = (M + 127) // 128
        bufs["stats_shift"] = prob.ints(-4, 4, N, scale=0.5)
        bufs["col_stats"] = parts = _sentinel((nparts + 1, N, 2), torch.float32, dev)

    # ---- the call ----
    want_ptrs = {k for k in PTRS if f.get(k) is not None}
    assert want_ptrs == set(bufs), (tag, want_ptrs ^ set(bufs))
    args = N_.GemmArgs(**{k: (bufs[k].data_ptr() if k in PTRS else v) for k, v in f.items()})
    for k in ("A", "B", "C"):
        assert bufs[k].data_ptr() % 16 == 0
    N_.check(N_.lib().dca_ops_gemm(ctypes.byref(args), N_.stream(dev)), "gemm " + tag)
    r = N_.GemmRoute()
    N_.check(N_.lib().dca_ops_gemm_last_route(ctypes.byref(r)), "gemm_last_route")
    want = GF.claims(case, form)
    got = {k: r.name.decode() if k == "name" else getattr(r, k) for k in want}
    if got != want:
        fails.append(f"{tag}: route {got}, claimed {want}")
        return

    # ---- output ----
    if form.amax:
        o = (view(parent) if form.wperm is not None else parent[idx, :N]).double()
        bound = 8 * U32 * mag + (HALF * ref.abs() if dt == torch.bfloat16 else 0.0)
        msg = _report(tag, (o - ref).abs(), bound)
        if msg:
            fails.append(msg)
        expected[idx, :N] = parent[idx, :N]   # the rest of the parent stays bitwise
    neq = _bits(parent) != _bits(expected)
    if bool(neq.any()):
        i = int(torch.nonzero(neq.reshape(-1))[0])
        fails.append(f"{tag}: {int(neq.sum())} of {neq.numel()} elements of the output parent {tuple(parent.shape)} "
                     f"differ; first at flat index {i}: got {parent.reshape(-1)[i].item()!r}, "
                     f"expected {expected.reshape(-1)[i].item()!r}")
    if form.mask and not (torch.equal(src, src0) and torch.equal(mask, mask0)):
        fails.append(f"{tag}: the masked source or its mask was written")

    # ---- statistics of the values as stored ----
    if form.stats:
        d = expected[idx, :N].double() - bufs["stats_shift"].double()
        tot = torch.stack([d.sum(0), (d * d).sum(0)], -1)
        dp = torch.cat([d, d.new_zeros(nparts * 128 - M, N)]).view(nparts, 128, N)
        rows64 = torch.stack([dp.sum(1), (dp * dp).sum(1)], -1)
        per_row = not case.kernel.startswith(("k_conv", "k_direct"))   # one partial row per 128 output rows
        # exact in fp32: per partial row; the row kernels write one row per workgroup, so there over all rows
        l1, l2 = (dp.abs().sum(1).max(), rows64[..., 1].max()) if per_row else (d.abs().sum(0).max(), tot[:, 1].max())
        assert float(4 * l1) < EXACT and float(16 * l2) < EXACT, tag
        if not torch.equal(_bits(parts[nparts]), _bits(_sentinel((N, 2), torch.float32, dev))):
            fails.append(f"{tag}: the row past the last partial row of col_stats was written")
        real = parts[:nparts]
        if not bool(torch.isfinite(real).all()):
            fails.append(f"{tag}: {int((~torch.isfinite(real)).sum())} col_stats values not written / not finite")
        elif not torch.equal(real.double().sum(0), tot):
            bad = (real.double().sum(0) != tot).any(-1)
            fails.append(f"{tag}: col_stats totals differ in {int(bad.sum())} of {N} columns")
        elif per_row and not torch.equal(real.double(), rows64):
            bad = (real.double() != rows64).any(-1).any(-1)
            fails.append(f"{tag}: col_stats partial rows {torch.nonzero(bad).view(-1)[:8].tolist()} differ")


@pytest.mark.parametrize("case", GF.CASES, ids=[c.id for c in GF.CASES])
def test_gemm_forms(gpu, case):
    probs, fails = {}, []
    for form in case.forms:
        tern = bool(form.stats)
        if tern not in probs:
            probs[tern] = _Problem(case, tern, gpu)
        _run_form(probs[tern], form, fails)
    assert not fails, "\n".join(fails)
