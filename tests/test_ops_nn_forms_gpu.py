"""The data-movement and head kernels of csrc/ops_nn.hip -- im2col / col2im, the four max-pool kernels, the global
average pool, cross-entropy, the small flat kernels, the input layouts, the weight-pack gathers and the fp8 quantisation --
against the float64 / integer references of tests/_nn_refs.py (proven on the CPU by tests/test_ops_nn_refs.py, which also
proves the exactness preconditions named below).  The C entry points are called directly wherever the Python wrapper
hides an output (argmax bytes, row losses, the ticket word).

Every output lives in a buffer pre-filled with 0xFF bytes (a NaN in bf16 / fp32) with a tail behind it, and is compared
whole: an element the kernel does not write fails, and so does a write past the end.  What is compared how:

  im2col          pure movement of distinct bf16 bit patterns: bitwise, the zero columns K..Kp and a sentinel row included.
  col2im          integer dcols in [-3, 3] (dx_old in +-8): every sum is a small integer, exact in fp32 in any order and
                  in bf16: bitwise.  The padding columns of dcols hold 7, so reading them shows.
  max pool        y is one of the window's bf16 values and the argmax byte the first maximum in tap order (inputs from
                  <= 4 values: ties in most windows): bitwise.  Backward from integer dy with the reference's taps:
                  bitwise, every input pixel written.  Random bf16 dy: bitwise where _nn_refs.fp32_sum_exact holds (all
                  partial sums multiples of the smallest addend's last bit and below 2^24 of them); everywhere
                  |dx - ref| <= 2^-8 |ref| + 3 2^-24 sum|terms| (half a bf16 ulp; at most 3 fp32 adds of the <= 4 addends
                  -- more than 4 addends only for the 3x3/1 and 5x5/2 windows, which run with integer dy).  NaN: y is NaN
                  exactly where the reference's is; the argmax is compared on the other windows.
  average pool    forward: HW - 1 sequential fp32 adds and one division, each within 2^-24 of a running value that is at
                  most sum|x|: |y - mean64| <= (HW + 2) 2^-24 mean|x|; the bf16 output adds half a bf16 ulp, 2^-8 |mean64|
                  (the 2^-8 of the fp32 error itself is inside the two spare 2^-24 mean|x| while HW + 2 <= 512).
                  Backward: dy / HW is exact for a power-of-two HW, so dx = bf16(dy / HW) bitwise; else one fp32 division
                  (2^-24) and the bf16 rounding (2^-8): |dx - dy / HW| <= (2^-8 + 2^-22) |dy / HW|.
  cross-entropy   see _ce_bounds.
  small kernels   cast_bf16 (round to nearest even, ties both ways, zeros, denormals, infinities), gather_cols, add_i64,
                  the runtime fill, k_scale_dev (a multiplication by 0.5), the two input layouts and the weight-pack
                  gathers are exact operations: bitwise (a NaN is compared by isnan).
  fp8             amax = max |x| exactly; q = torch's float8_e4m3fn of clamp(fp32(x) sc, +-448) with sc = 448 / amax
                  evaluated in fp32 (correctly rounded, as the kernel's division is compiled); the cases with amax =
                  448 2^k need no assumption about the division.

Each check prints its largest error / bound ratio (0 or 1 for a bitwise one) under pytest -s.

(The module's name puts it after tests/test_ddp_engine_gpu.py and tests/test_multigpu.py in pytest's order: those spawn
8 rank processes on one GPU, and until they have run, the pytest process itself should hold no GPU context.)"""
import math

import pytest
import torch

import _nn_refs as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
HALF = 2.0 ** -8     # half a bf16 ulp, relative
U32 = 2.0 ** -24     # one fp32 rounding, relative
ULP32 = 2.0 ** -23   # one fp32 ulp, relative
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _N():
    from distributeddataparallel_cifar10_amd.ops import _native
    return _native


def _F():
    from distributeddataparallel_cifar10_amd.ops import functional
    return functional


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
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound; worst at flat index {i}: "
                             f"error {err.reshape(-1)[i].item():.6g}, bound {bound.reshape(-1)[i].item():.6g}")


class Out:
    """n elements of dtype on the device inside a buffer of 0xFF bytes with a tail of `tail` more elements."""

    def __init__(self, n, dtype, gpu, tail=32, init=None):
        self.n, self.dtype = n, dtype
        self.isz = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((n + tail) * self.isz,), 0xFF, dtype=U8, device=gpu)
        self.t = self.raw.view(dtype)[:n]
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))

    def host(self):
        torch.cuda.synchronize()
        return self.raw.cpu().view(self.dtype)[:self.n].clone()

    def tail_intact(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw.cpu()[self.n * self.isz:] == 0xFF).all()), f"{what}: written past the end"

    def check(self, what, ref, ignore=None):
        """The whole buffer, tail included, against ref (host, n elements of the dtype) bit for bit; ignore: a host
        bool mask of elements left out of the comparison."""
        ref = ref.contiguous().reshape(-1)
        assert ref.dtype == self.dtype and ref.numel() == self.n, (ref.dtype, ref.numel(), self.n)
        exp = torch.full((self.raw.numel(),), 0xFF, dtype=U8)
        exp[:self.n * self.isz] = ref.view(U8)
        torch.cuda.synchronize()
        bad = self.raw.cpu().view(_INT[self.isz]) != exp.view(_INT[self.isz])
        if ignore is not None:
            bad[:self.n] &= ~ignore.reshape(-1)
        print(f"ratio {what} {float(bad.any()):.4f}")
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at "
                                     f"{int(bad.nonzero()[0])} (the tail starts at {self.n})")


def _conv_geom(geom):
    n, h, w, c, k, s, p = geom
    kk = k * k * c
    return _N().ConvGeom(N=n, H=h, W=w, C=c, KH=k, KW=k, stride=s, pad=p, Ho=R.out_size(h, k, s, p),
                         Wo=R.out_size(w, k, s, p), K=kk, Kp=(kk + 7) // 8 * 8)


# ---------------------------------------------------------------------------------------------------------------------
# im2col / col2im
# ---------------------------------------------------------------------------------------------------------------------
def _run_im2col(gpu, geom, wider=0):
    N = _N()
    n, h, w, c, k, s, p = geom
    g = _conv_geom(geom)
    g.Kp += wider
    xi = (torch.arange(n * h * w * c) + 1).to(torch.int16).view(n, h, w, c)     # distinct, non-zero bit patterns
    ref = R.im2col(xi, k, s, p, kp=g.Kp)
    assert ref.shape == (n * g.Ho * g.Wo, g.Kp) and not bool(ref[:, g.K:].any())
    x = xi.view(BF).to(gpu)
    out = Out(ref.numel(), BF, gpu, tail=g.Kp)                                  # a sentinel row behind the last
    N.check(N.lib().dca_ops_im2col(N.ptr(x), N.ptr(out.t), g, N.stream(gpu)), "im2col")
    out.check(f"im2col {geom} Kp {g.Kp}", ref.view(BF))


def _run_col2im(gpu, geom, acc, wider=0):
    N = _N()
    n, h, w, c, k, s, p = geom
    g = _conv_geom(geom)
    g.Kp += wider
    rng = R.gen(sum(geom))
    M = n * g.Ho * g.Wo
    d = torch.full((M, g.Kp), 7.0, dtype=F64)
    d[:, :g.K] = R.randint(rng, -3, 3, (M, g.K))
    old = R.randint(rng, -8, 8, (n, h, w, c))
    ref = R.col2im(d, geom, old if acc else None)
    dcols = d.to(BF).to(gpu)
    out = Out(n * h * w * c, BF, gpu, init=old if acc else None)
    N.check(N.lib().dca_ops_col2im(N.ptr(dcols), N.ptr(out.t), g, acc, N.stream(gpu)), "col2im")
    out.check(f"col2im {geom} Kp {g.Kp} accumulate {acc}", ref.to(BF))


@pytest.mark.parametrize("geom", R.IM2COL_GEOMS, ids=str)
def test_im2col(gpu, geom):
    _run_im2col(gpu, geom)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("geom", R.COL2IM_GEOMS, ids=str)
def test_col2im(gpu, geom, acc):
    _run_col2im(gpu, geom, acc)


@pytest.mark.parametrize("geom", R.IM2COL_GEOMS[:2], ids=str)
def test_im2col_col2im_wider_kp(gpu, geom):
    """C % 8 == 0 makes K a multiple of 8 and Kp = K in every use so far; the launchers admit any Kp >= K, and only a
    wider row reaches the 16-byte path's own k0 < K guard (im2col: the extra group is zero; col2im: it is not read)."""
    assert geom[3] % 8 == 0
    _run_im2col(gpu, geom, wider=8)
    _run_col2im(gpu, geom, 0, wider=8)


# ---------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_geom(case):
    k, s, p, h, w, c = case
    return _N().PoolGeom(N=R.POOL_N, H=h, W=w, C=c, K=k, S=s, P=p, Ho=R.out_size(h, k, s, p), Wo=R.out_size(w, k, s, p))


def _pool_id(case):
    return "-".join(map(str, case)) + "-" + R.pool_family(*case)


def _pool_fwd(gpu, case, x64):
    N = _N()
    g = _pool_geom(case)
    n_out = g.N * g.Ho * g.Wo * g.C
    x = x64.to(BF).to(gpu)
    y, arg = Out(n_out, BF, gpu), Out(n_out, U8, gpu)
    N.check(N.lib().dca_ops_maxpool_fwd(N.ptr(x), N.ptr(y.t), N.ptr(arg.t), g, N.stream(gpu)), "maxpool_fwd")
    return y, arg


def _pool_bwd(gpu, case, dy64, tap):
    N = _N()
    g = _pool_geom(case)
    dx = Out(g.N * g.H * g.W * g.C, BF, gpu)
    dy, arg = dy64.to(BF).to(gpu), tap.to(gpu)
    N.check(N.lib().dca_ops_maxpool_bwd(N.ptr(dy), N.ptr(arg), N.ptr(dx.t), g, N.stream(gpu)), "maxpool_bwd")
    return dx


@pytest.mark.parametrize("case", R.POOL_CASES, ids=_pool_id)
def test_maxpool_ties(gpu, case):
    k, s, p, h, w, c = case
    x64 = R.pool_input(case)
    ry, rtap = R.maxpool_fwd(x64, k, s, p)
    y, arg = _pool_fwd(gpu, case, x64)
    y.check(f"maxpool {_pool_id(case)} y", ry.to(BF))
    arg.check(f"maxpool {_pool_id(case)} argmax", rtap)
    dy64 = R.randint(R.gen(5 + sum(case)), -3, 3, tuple(ry.shape))
    rdx = R.maxpool_bwd(dy64, rtap, (R.POOL_N, h, w, c, k, s, p))[0]
    _pool_bwd(gpu, case, dy64, rtap).check(f"maxpool {_pool_id(case)} dx", rdx.to(BF))


@pytest.mark.parametrize("case", R.POOL_RANDOM, ids=_pool_id)
def test_maxpool_random(gpu, case):
    k, s, p, h, w, c = case
    x64 = R.pool_input(case, random=True)
    ry, rtap = R.maxpool_fwd(x64, k, s, p)
    y, arg = _pool_fwd(gpu, case, x64)
    y.check(f"maxpool randn {_pool_id(case)} y", ry.to(BF))
    arg.check(f"maxpool randn {_pool_id(case)} argmax", rtap)
    dy64 = torch.randn(tuple(ry.shape), generator=R.gen(9)).to(BF).to(F64)
    rdx, sab, mn = R.maxpool_bwd(dy64, rtap, (R.POOL_N, h, w, c, k, s, p))
    exact = R.fp32_sum_exact(sab, mn)
    dx = _pool_bwd(gpu, case, dy64, rtap)
    dx.tail_intact("maxpool dx")
    got = dx.host().view(rdx.shape)
    _report(f"maxpool randn {_pool_id(case)} dx", (got.to(F64) - rdx).abs(), HALF * rdx.abs() + 3 * U32 * sab)
    print(f"exact in fp32: {float(exact.double().mean()):.3f} of the pixels")
    dx.check(f"maxpool randn {_pool_id(case)} dx where exact", rdx.to(BF), ignore=~exact)


@pytest.mark.parametrize("case", R.POOL_RANDOM, ids=_pool_id)
def test_maxpool_nan(gpu, case):
    """NaNs at a window's first tap, at a window's last tap and in a window that reaches into the padding."""
    k, s, p, h, w, c = case
    x64 = R.pool_input(case, random=True)
    nan = float("nan")
    x64[0, 1, 1, 0] = nan      # first tap of window (1, 1), last tap of the border window (0, 0)
    x64[0, 3, 3, 1] = nan      # last tap of window (1, 1), first tap of window (2, 2)
    x64[1, 0, 0, 2] = nan      # the centre of the padded corner window
    x64[1, 2, 5, 3] = x64[1, 2, 6, 3] = nan    # two in one window: the first wins
    ry, rtap = R.maxpool_fwd(x64, k, s, p)
    isn = torch.isnan(ry)
    assert 4 <= int(isn.sum()) < isn.numel() // 4
    y, arg = _pool_fwd(gpu, case, x64)
    y.tail_intact("maxpool y")
    got = y.host().view(ry.shape)
    assert torch.equal(torch.isnan(got), isn), "y is not NaN exactly where the reference's is"
    y.check(f"maxpool NaN {_pool_id(case)} y", ry.to(BF), ignore=isn)
    arg.check(f"maxpool NaN {_pool_id(case)} argmax", rtap, ignore=isn)


# ---------------------------------------------------------------------------------------------------------------------
# global average pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=str)
def test_avgpool_fwd(gpu, shape, out_bf16):
    N = _N()
    n, hw, c = shape
    x = (torch.randn(n, hw, c, generator=R.gen(hw + c)) + 0.25).to(BF)
    ref = R.avgpool_fwd(x)
    bound = (hw + 2) * U32 * x.to(F64).abs().mean(1) + (HALF * ref.abs() if out_bf16 else 0)
    y = Out(n * c, BF if out_bf16 else F32, gpu)
    xd = x.to(gpu)      # (a local: the device copy must outlive the launch)
    N.check(N.lib().dca_ops_avgpool_fwd(N.ptr(xd), N.ptr(y.t), n, hw, c, out_bf16, N.stream(gpu)), "avgpool_fwd")
    y.tail_intact("avgpool y")
    _report(f"avgpool fwd {shape} bf16 {out_bf16}", (y.host().view(n, c).to(F64) - ref).abs(), bound)


@pytest.mark.parametrize("dy_bf16", [0, 1])
@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=str)
def test_avgpool_bwd(gpu, shape, dy_bf16):
    """C % 8 == 0: k_avgpool_bwd8<float> / <bf16_t>; else the scalar k_avgpool_bwd (fp32 dy only: the launcher rejects a
    bf16 dy there, and global_avg_pool's autograd converts it -- test_avgpool_autograd_bf16_dy_odd_channels)."""
    N = _N()
    n, hw, c = shape
    if dy_bf16 and c % 8:
        dy = torch.zeros(n, c, dtype=BF, device=gpu)
        dx = torch.empty(n, hw, c, dtype=BF, device=gpu)
        assert N.lib().dca_ops_avgpool_bwd(N.ptr(dy), N.ptr(dx), n, hw, c, 1, N.stream(gpu)) != 0   # refused, no launch
        return
    dy = torch.randn(n, c, generator=R.gen(hw * c))
    dy = dy.to(BF) if dy_bf16 else dy
    ref = R.avgpool_bwd(dy, hw)
    dx = Out(n * hw * c, BF, gpu)
    dyd = dy.to(gpu)
    N.check(N.lib().dca_ops_avgpool_bwd(N.ptr(dyd), N.ptr(dx.t), n, hw, c, dy_bf16, N.stream(gpu)), "avgpool_bwd")
    if hw & (hw - 1) == 0:
        dx.check(f"avgpool bwd {shape} bf16 {dy_bf16}", ref.to(BF))
    else:
        dx.tail_intact("avgpool dx")
        _report(f"avgpool bwd {shape} bf16 {dy_bf16}", (dx.host().view(ref.shape).to(F64) - ref).abs(),
                (HALF + 4 * U32) * ref.abs())


def test_avgpool_autograd_bf16_dy_odd_channels(gpu):
    """A bf16 dy with C % 8 != 0 through global_avg_pool's autograd takes the fp32 route and still matches."""
    F = _F()
    x = torch.randn(2, 4, 4, 5, generator=R.gen(1)).to(BF).to(gpu).requires_grad_(True)
    dy = torch.randn(2, 5, generator=R.gen(2)).to(BF)
    y = F.global_avg_pool(x, out_dtype=BF)
    assert y.dtype == BF
    y.backward(dy.to(gpu))
    ref = R.avgpool_bwd(dy, 16).view(2, 4, 4, 5).to(BF)
    bad = R.bf16_bits(x.grad.cpu()) != R.bf16_bits(ref)
    print(f"ratio avgpool autograd {float(bad.any()):.4f}")
    assert not bool(bad.any())


# ---------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def _ce_bounds(x, y, gs):
    """float64 references and error bounds of k_cross_entropy's outputs for logits x (fp32, host), labels y and the
    fp32 grad_scale gs.  With m the row maximum (exact), t_k = row[k] - m in [-100, 0] and u = 2^-24:

      e_k   __expf(t) is v_exp_f32 (1 ulp = 2u) of t log2(e) rounded once, on a t that is itself one fp32 subtraction:
            the exponent's error is within 3u |t| log2(e) binary orders, i.e. 3u |t| relative, so the relative error of
            e_k is rho(t) <= (2 |t| + 2) 2^-23 (taken with that spare); a result below 2^-126 may be flushed: an
            absolute 2^-126 per term.
      s     the sum of the K positive terms, ceil(K / 64) serial adds per lane and a 6-level shuffle tree: relative
            (ceil(K / 64) + 6) u on top of the terms' own errors:  Rs = sum_k rho(t_k) e_k / s + (ceil(K / 64) + 6) u
            + K 2^-126 / s  (s >= 1: the maximum's term is 1).
      log   |log(s (1 + r)) - log s| <= r / (1 - r); __logf adds 1 ulp of its result.
      loss  lse = m + log rounds once at max(|lse|, |row[y]|) at most, and lse - row[y] once at |loss|.
      dl    p_k = e_k / s: rho(t_k) + Rs + 3u (the reciprocal within 1 ulp and the product), then the subtraction of
            the one-hot and the multiplication by grad_scale, one rounding each of |p - onehot|: relative 2u; a flushed
            term adds 2^-126.
      mean  ceil(B / 64) serial adds per lane, the 6-level tree and the division by B: (ceil(B / 64) + 7) u of
            mean|loss|, on top of the mean of the rows' own bounds.
    A factor 1 + 1e-3 covers the products of these terms (each below 3e-5)."""
    B, K = x.shape
    loss, mean, dl, lse, s, p = R.cross_entropy(x, y, gs)
    x64 = x.to(F64)
    t = x64 - x64.max(1, keepdim=True).values
    assert float(t.abs().max()) <= R.CE_T_MAX
    rho, e = (2 * t.abs() + 2) * ULP32, torch.exp(t)
    rs = (rho * e).sum(1) / s + (math.ceil(K / 64) + 6) * U32 + K * 2.0 ** -126 / s
    a = rs / (1 - rs) + ULP32 * torch.log(s)
    xy = x64.gather(1, y.clamp(0, K - 1)[:, None]).squeeze(1)
    so = 1 + 1e-3
    e_loss = so * (a + U32 * torch.maximum(lse.abs(), xy.abs()) + U32 * loss.abs())
    onehot = torch.zeros_like(p).scatter_(1, y.clamp(0, K - 1)[:, None], 1.0)
    e_dl = so * gs * (p * (rho + rs[:, None] + 3 * U32) + 2 * U32 * (p - onehot).abs() + 2.0 ** -126)
    e_mean = e_loss.mean() + so * (math.ceil(B / 64) + 7) * U32 * (loss.abs() + e_loss).mean()
    return loss, e_loss, dl, e_dl, mean, e_mean


def _ce_launch(gpu, x, y, gs, want_dl=True, want_mean=True, ticket=None):
    N = _N()
    B, K = x.shape
    loss, dl, mean = Out(B, F32, gpu), Out(B * K, F32, gpu), Out(1, F32, gpu)
    xd, yd = x.to(gpu), y.to(gpu)      # (locals: both device copies must stay allocated until the launch has run)
    N.check(N.lib().dca_ops_cross_entropy(N.ptr(xd), N.ptr(yd), N.ptr(loss.t),
                                          N.ptr(dl.t) if want_dl else None, B, K, gs,
                                          N.ptr(mean.t) if want_mean else None, N.ptr(ticket) if want_mean else None,
                                          N.stream(gpu)), "cross_entropy")
    return loss, dl, mean


@pytest.mark.parametrize("case", R.CE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_cross_entropy(gpu, case):
    B, K, mode = case
    x, y = R.ce_inputs(B, K, mode)
    gs = 0.25 if case == (33, 10, "ends") else torch.tensor(1.0 / B, dtype=F32).item()
    rl, el, rd, ed, rm, em = _ce_bounds(x, y, gs)
    ticket = torch.zeros(4, dtype=torch.int32, device=gpu)
    loss, dl, mean = _ce_launch(gpu, x, y, gs, ticket=ticket)
    for o in (loss, dl, mean):
        o.tail_intact("cross_entropy")
    tag = f"cross_entropy {B}x{K} {mode}"
    _report(f"{tag} loss", (loss.host().to(F64) - rl).abs(), el)
    _report(f"{tag} dlogits", (dl.host().view(B, K).to(F64) - rd).abs(), ed)
    _report(f"{tag} mean", (mean.host().to(F64) - rm).abs().view(1), em.view(1))
    assert not bool(ticket.cpu().any()), "the ticket word is not reset"
    # the same word again: the same bits
    loss2, dl2, mean2 = _ce_launch(gpu, x, y, gs, ticket=ticket)
    loss2.check(f"{tag} loss, second launch", loss.host())
    dl2.check(f"{tag} dlogits, second launch", dl.host())
    mean2.check(f"{tag} mean, second launch", mean.host())
    assert not bool(ticket.cpu().any())
    # dlogits = nullptr; loss_mean = ticket = nullptr (the mean output stays untouched)
    loss3, dl3, mean3 = _ce_launch(gpu, x, y, gs, want_dl=False, ticket=ticket)
    loss3.check(f"{tag} loss, no dlogits", loss.host())
    mean3.check(f"{tag} mean, no dlogits", mean.host())
    dl3.tail_intact("dlogits")
    assert bool((dl3.raw == 0xFF).all())
    loss4, dl4, mean4 = _ce_launch(gpu, x, y, gs, want_mean=False)
    loss4.check(f"{tag} loss, no mean", loss.host())
    dl4.check(f"{tag} dlogits, no mean", dl.host())
    assert bool((mean4.raw == 0xFF).all()) and not bool(ticket.cpu().any())


def test_scale_dev(gpu):
    """k_scale_dev through cross_entropy(...).backward(g) with g = 0.5: dlogits 0.5, an exact multiplication."""
    F = _F()
    B, K = 33, 10
    x, y = R.ce_inputs(B, K, "ends")
    gs = torch.tensor(1.0 / B, dtype=F32).item()
    _, dl, _ = _ce_launch(gpu, x, y, gs, ticket=torch.zeros(1, dtype=torch.int32, device=gpu))
    logits = x.to(gpu).requires_grad_(True)
    loss = F.cross_entropy(logits, y.to(gpu))
    loss.backward(torch.tensor(0.5, device=gpu))
    bad = logits.grad.cpu().view(torch.int32) != (dl.host().view(B, K) * 0.5).view(torch.int32)
    print(f"ratio scale_dev {float(bad.any()):.4f}")
    assert not bool(bad.any())


# ---------------------------------------------------------------------------------------------------------------------
# small flat kernels
# ---------------------------------------------------------------------------------------------------------------------
def _cmp_bits(what, got, ref):
    bad = got.contiguous().view(_INT[got.element_size()]) != ref.contiguous().view(_INT[ref.element_size()])
    print(f"ratio {what} {float(bad.any()):.4f}")
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {int(bad.nonzero()[0][0])}"


@pytest.mark.parametrize("n", [1, 255, 257, 10001])
def test_cast_bf16(gpu, n):
    F = _F()
    special = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000 - (1 << 32), 0xBF818000 - (1 << 32), 0x3F808001,
                            0x3F817FFF, 0, 0x80000000 - (1 << 32), 1, 0x00008000, 0x00018000, 0x007FFFFF,
                            0x80018000 - (1 << 32), 0x7F800000, 0xFF800000 - (1 << 32), 0x7F7FFFFF, 0x7FC00000],
                           dtype=torch.int32).view(F32)
    x = torch.randn(n, generator=R.gen(n)) * 100
    if n == 1:
        x[0] = special[1]      # a tie that rounds up to the even neighbour
    else:
        x[n - len(special):] = special
    y = F.cast_bf16(x.to(gpu))
    assert y.shape == x.shape and y.dtype == BF
    got, ref = y.cpu(), x.to(BF)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    _cmp_bits(f"cast_bf16 {n}", torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref))


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("L", [1, 64, 70])
@pytest.mark.parametrize("rows", [1, 37])
def test_gather_cols(gpu, rows, L, acc):
    F = _F()
    S = 50
    g = R.gen(rows + L)
    idx = torch.randint(0, S, (L,), generator=g)
    idx[0] = S - 1
    if L > 1:
        idx[-1] = 0
        idx[L // 2] = idx[L // 2 - 1]          # a repeat
        assert len(set(idx.tolist())) < L and {0, S - 1} <= set(idx.tolist())
    src = R.randint(g, -50, 50, (rows, S)).float() if acc else torch.randn(rows, S, generator=g)
    old = R.randint(g, -50, 50, (rows, L)).float()
    out = Out(rows * L, F32, gpu, init=old if acc else None)
    F.gather_cols(src.to(gpu), idx.to(gpu), out.t.view(rows, L), accumulate=acc)
    out.check(f"gather_cols {rows}x{L} accumulate {acc}", src[:, idx] + old if acc else src[:, idx])


@pytest.mark.parametrize("n", [1, 64, 65, 161])
def test_add_one_i64(gpu, n):
    F = _F()
    starts = [0, 2 ** 32 - 1, 2 ** 40, -1, 7]
    big = torch.full((3 * n + 5,), 0x0123456789ABCDEF, dtype=torch.int64)
    pos = 1 + 3 * torch.arange(n)
    big[pos] = torch.tensor([starts[i % len(starts)] for i in range(n)], dtype=torch.int64)
    ref = big.clone()
    ref[pos] += 1
    dev = big.to(gpu)
    ptrs = (dev.data_ptr() + 8 * pos).to(gpu)
    F.add_one_i64(ptrs, n)
    torch.cuda.synchronize()
    _cmp_bits(f"add_one_i64 {n}", dev.cpu(), ref)


def test_zeros_bf16(gpu):
    F = _F()
    shape = (3, 37, 5)
    stale = torch.full(shape, float("nan"), dtype=BF, device=gpu)    # the block the allocator may hand back
    torch.cuda.synchronize()
    del stale
    z = F.zeros_bf16(*shape, device=gpu)
    assert z.shape == shape and z.dtype == BF and z.numel() % 2 == 1
    assert not bool(R.bf16_bits(z.cpu()).any())


@pytest.mark.parametrize("c", [1, 3, 8])
def test_nchw_to_nhwc8(gpu, c):
    F = _F()
    x = torch.randn(2, c, 5, 7, generator=R.gen(c))
    _cmp_bits(f"nchw_to_nhwc8 C {c}", F.nchw_to_nhwc8(x.to(gpu)).cpu(), R.nchw_to_nhwc8(x))


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", [(10, 14), (9, 11)])
def test_nchw_to_s2d16_stem7(gpu, c, hw):
    """The wrapper's 7x7/2/3 stem: P = 4, [N, Ho + 3, Wo + 3, 16]."""
    F = _F()
    h, w = hw
    x = torch.randn(2, c, h, w, generator=R.gen(c + h))
    y = F.nchw_to_s2d16(x.to(gpu))
    hs, ws = R.out_size(h, 7, 2, 3) + 3, R.out_size(w, 7, 2, 3) + 3
    assert F.S2D_PAD == 4 and F.S2D_TAPS == 4
    _cmp_bits(f"nchw_to_s2d16 7x7 C {c} {hw}", y.cpu(), R.nchw_to_s2d16(x, hs, ws, 4))


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", [(8, 6), (7, 9)])
def test_nchw_to_s2d16_stem3(gpu, c, hw):
    """A 3x3/2/1 stem by the kernel comment's rule: P = padding + 1 = 2, 2x2 taps, [N, Ho + 1, Wo + 1, 16]."""
    N = _N()
    h, w = hw
    x = torch.randn(2, c, h, w, generator=R.gen(c + h))
    hs, ws = R.out_size(h, 3, 2, 1) + 1, R.out_size(w, 3, 2, 1) + 1
    y = Out(2 * hs * ws * 16, BF, gpu)
    xd = x.to(gpu)
    N.check(N.lib().dca_ops_nchw_to_s2d16(N.ptr(xd), N.ptr(y.t), 2, c, h, w, hs, ws, 2, N.stream(gpu)),
            "nchw_to_s2d16")
    y.check(f"nchw_to_s2d16 3x3 C {c} {hw}", R.nchw_to_s2d16(x, hs, ws, 2))


def test_weight_pack_gathers(gpu):
    """k_pack_gather: the parity-class matrices of a 3x3/2/1 conv, the W^T of a 1x1/2/0 one (k_pack_weights' dgrad), and
    the space-to-depth stem matrix, against the docstring formulas."""
    F = _F()
    torch.manual_seed(3)
    conv3 = torch.nn.Conv2d(8, 16, 3, stride=2, padding=1, bias=False).to(gpu)
    conv1 = torch.nn.Conv2d(8, 16, 1, stride=2, padding=0, bias=False).to(gpu)
    conv7 = torch.nn.Conv2d(3, 16, 7, stride=2, padding=3, bias=False).to(gpu)
    pack = F.WeightPack([conv3, conv1, conv7], (), [conv7])
    e3, e1, e7 = pack.get(conv3), pack.get(conv1), pack.get(conv7)
    assert len(e3["classes"]) == 4 and e1["classes"] is None and e1["dgrad"] is not None and e7["s2d"] is not None
    for t in [cl[5] for cl in e3["classes"]] + [e1["dgrad"], e7["fwd"]]:
        t.fill_(float("nan"))
    pack.pack()
    torch.cuda.synchronize()
    ref3 = R.parity_classes(conv3.weight.detach().cpu(), 1)
    for ph, pw, nkh, nkw, pad, out, _ in e3["classes"]:
        khl, kwl, pads, m = ref3[(ph, pw)]
        assert (nkh, nkw, (pad, pad)) == (len(khl), len(kwl), pads)
        _cmp_bits(f"parity class ({ph}, {pw})", out.cpu(), m.float().to(BF))
    ref1 = R.parity_classes(conv1.weight.detach().cpu(), 0)
    assert list(ref1) == [(0, 0)]
    _cmp_bits("1x1/2 class (0, 0)", e1["dgrad"].cpu(), ref1[(0, 0)][3].float().to(BF))
    idx = e7["s2d"]["fwd_idx"].cpu().long()
    wflat = conv7.weight.detach().cpu().reshape(-1)
    ref7 = torch.where(idx >= 0, wflat[idx.clamp_min(0)], torch.zeros(())).to(BF).view(e7["fwd"].shape)
    assert bool((idx < 0).any()) and bool((idx >= 0).any())
    _cmp_bits("s2d stem matrix", e7["fwd"].cpu(), ref7)


# ---------------------------------------------------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.FP8_KINDS)
@pytest.mark.parametrize("is_f32", [0, 1])
@pytest.mark.parametrize("n", R.FP8_SIZES)
def test_quant_fp8(gpu, n, is_f32, kind):
    N = _N()
    x = R.fp8_input(n, kind)
    bits, rq = R.quant_fp8(x)
    xd = (x if is_f32 else x.to(BF)).to(gpu)
    q, amax = Out(n, U8, gpu), Out(1, torch.int32, gpu)
    N.check(N.lib().dca_ops_quant_fp8(N.ptr(xd), is_f32, n, N.ptr(q.t), N.ptr(amax.t), N.stream(gpu)), "quant_fp8")
    amax.check(f"quant_fp8 {n} {kind} f32 {is_f32} amax", torch.tensor([bits], dtype=torch.int32))
    q.check(f"quant_fp8 {n} {kind} f32 {is_f32} q", rq)


def test_quantize_fp8_wrapper_2d(gpu):
    F = _F()
    x = R.fp8_input(4099, "randn")[:4092].view(33, 124)
    bits, rq = R.quant_fp8(x)
    q, amax = F.quantize_fp8(x.to(BF).to(gpu))
    assert q.shape == x.shape and int(amax.cpu()) == bits
    _cmp_bits("quantize_fp8 33x124", q.cpu(), rq)


@pytest.mark.parametrize("a,b,extra", [(3.5, 0.75, 1.0), (0.0, 2.0, 0.5), (1.25, 0.0, 2.0), (0.0, 0.0, 3.0),
                                       (448.0, 7.0, 0.125)])
def test_fp8_alpha(gpu, a, b, extra):
    F = _F()
    ta, tb = torch.tensor([a], dtype=F32), torch.tensor([b], dtype=F32)
    got = F.fp8_alpha(ta.view(torch.int32).to(gpu), tb.view(torch.int32).to(gpu), extra)
    _cmp_bits(f"fp8_alpha {a} {b} {extra}", got.cpu(), R.fp8_alpha(ta[0], tb[0], extra).view(1))
