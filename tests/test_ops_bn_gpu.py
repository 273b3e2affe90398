"""Every dispatched form of the BatchNorm passes (csrc/ops_nn.hip k_bn_stats / k_bn_fin_ticket / k_bn_apply /
k_bn_bwd_stats / k_bn_bwd_apply, chosen by csrc/ops_api.hip bn_plan) against float64, per element and per channel.

Each case first asserts, through dca_ops_bn_plan, the instantiation it claims to cover, then compares with a float64
reference computed by torch on the same device from the same bf16 tensors and fp32 parameters:

    mean, biased var, invstd = (var + eps)^-1/2;  sc = invstd gamma, sh = beta - mean sc
    pre = x sc + sh (+ r' if res_mode 2);  out = relu?(pre) (+ r' if res_mode 1)
    r' = r, or r normalised on the fly with its own float64 statistics

Tolerances (derived from the number formats and the kernels' operation counts, never from what the kernels return):

  statistics    the deepest serial fp32 chain of k_bn_stats + k_bn_fin_ticket (and of the backward sums) is under 150
                adds of 2^-24 each: K = 2e-5 covers it twice.  Per channel |mean - mean64| <= K E|x - shift|,
                |var - var64| <= K (E(x - shift)^2 + 2 |dm| E|x - shift|); running statistics the same, scaled by
                the momentum.  Added to each: the fp32 roundings of the stored value itself (mean: one; var read back
                from the stored invstd: 8; a running value's own (1 - m) old + m new: 4), which only matter where
                the K term vanishes (M = 1).
  output        E = 4e-5 (|x sc| + |sh| + |r'|) per element, the fp32 evaluation error including that of the
                statistics; |y - out64| <= 2^-8 |out64| + (1 + 2^-8) E, 2^-8 being half a bf16 ulp.  ReLU is
                1-Lipschitz: no element is excluded.
  mask          bit j of byte o >> 3 == (y_kernel > 0), exactly.
  fp8 copy      q == torch's float8_e4m3fn of clamp(y_kernel 448 / amax_prev, +-448) and amax_out == max|y_kernel|,
                bitwise; amax_prev == 0 means scale 1.
  backward      runs on stats = fp32(mean64, invstd64), so it is tested on its own (its reference takes those fp32
                values).  dz64 = dy [pre64 > 0] (dy for BWD_PLAIN, dy bit for BWD_MASK with bits the test draws).
                A = {|pre64| <= E} is where the kernel may take either branch; |A| <= 1e-3 of the elements,
                asserted on the reference alone.  (A is taken no larger than E allows: with the smaller of E and
                the same bound written for the backward's own evaluation, 4e-5 (|xhat gamma| + |beta| + |r|).  At
                M = 1 the variance is 0, x sc and sh cancel to beta at 300 times its size, and E alone would call
                a third of the elements ambiguous, where the backward, with xhat = 0, has no doubt at all.)  Per channel |d dbeta| <= K sum|dz| + sum_A|dy|, |d dgamma| <=
                K sum|dz xhat| + sum_A|dy xhat| (accumulate = 1: plus the one fp32 add into the pre-filled view).
                dx per element: 2^-8 |dx64| + the two sum tolerances through gamma invstd (. / M) + 4 fp32 ulps of
                |ca dz| + |cb x| + |cd| (the kernel's ca dz + cb x + cd form); elements of A must match one of the
                two candidates.  dr == bf16(dz) bitwise (either candidate in A).

Outputs are pre-filled with NaN / 0xFF, so an element a kernel does not write fails.  Each check prints its largest
error / bound ratio (pytest -s).

(The module's name puts it after tests/test_ddp_engine_gpu.py and tests/test_multigpu.py in pytest's order: those spawn
8 rank processes on one GPU, and until they have run, the pytest process itself should hold no GPU context -- a ninth
process with queues on the device.)"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 2e-5
HALF = 2.0 ** -8     # half a bf16 ulp, relative
U32 = 2.0 ** -24     # one fp32 rounding, relative
ULP32 = 2.0 ** -23   # one fp32 ulp, relative
EPS = torch.tensor(1e-5, dtype=torch.float32).item()   # as the kernels receive them
MOM = torch.tensor(0.1, dtype=torch.float32).item()
PLAIN, RELU, RES, MASK = 0, 1, 2, 3
A_CAP = 1e-3


def _N():
    from distributeddataparallel_cifar10_amd.ops import _native
    return _native


def _F():
    from distributeddataparallel_cifar10_amd.ops import functional
    return functional


def _assert_plan(M, C, relu, res_mode, mask, raff, lanes, apply, bwd):
    """apply = (rows, nt) of k_bn_apply; bwd = (mode, stats nt, apply rows, apply nt) of the backward kernels."""
    p = _N().bn_plan(M, C, relu, res_mode, mask, raff)
    got = (p.lanes, (p.apply_rows, p.apply_nt), p.raff, (p.bwd_mode, p.bwd_stats_nt, p.bwd_rows, p.bwd_apply_nt))
    assert got == (lanes, apply, int(raff), bwd), (M, C, got)


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


@functools.lru_cache(maxsize=1)   # one shape's tensors at a time: the previous shape's are freed
def _inputs(M, C, dev):
    # small shapes are drawn on the host (the same numbers everywhere), the 2^25+ ones on the device
    gdev = dev if M * C > 1 << 20 else "cpu"
    g = torch.Generator(device=gdev).manual_seed(1000003 * C + M)

    def rn():
        return torch.randn(M, C, generator=g, device=gdev).to(dev)

    def ru(n, lo, hi):
        return (torch.rand(n, generator=g, device=gdev) * (hi - lo) + lo).to(dev).contiguous()
    d = dict(x=(rn() * 2 + 0.5).bfloat16(), r=rn().bfloat16(), dy=rn().bfloat16(),
             gamma=ru(C, 0.5, 1.5), beta=ru(C, -0.2, 0.2), rgamma=ru(C, 0.5, 1.5), rbeta=ru(C, -0.2, 0.2),
             g0=ru(C, -1.0, 1.0), b0=ru(C, -1.0, 1.0))
    d["bits"] = (torch.rand(M, C, generator=g, device=gdev) > 0.4).to(dev)
    d["mask"] = _pack_bits(d["bits"])
    return d


def _pack_bits(bits):
    """[M, C] bool -> [M C / 8] bytes, bit j of byte o >> 3 = element o = 8 (o >> 3) + j."""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=bits.device)
    return (bits.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8).contiguous()


def _stats64(x64):
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    return mean, var


def _parts128(x, shift):
    """What the conv GEMM's epilogue hands dca_ops_bn_fwd_parts: per 128 rows, the sums of x - shift and its square
    (here summed in float64, then rounded to fp32)."""
    d = x.double() - shift.double()
    M, C = d.shape
    n = (M + 127) // 128
    if n * 128 != M:
        d = torch.cat([d, d.new_zeros(n * 128 - M, C)])
    d = d.view(n, 128, C)
    return torch.stack([d.sum(1), (d * d).sum(1)], -1).float().contiguous(), n


def _check_stats(tag, stats, rm_new, rv_new, x64, rm_old, rv_old, momentum=MOM):
    """The (mean, invstd) a training forward left in ``stats`` and its running-statistics update, per channel."""
    M = x64.shape[0]
    shift, rv0 = rm_old.double(), rv_old.double()
    mean64, var64 = _stats64(x64)
    d = x64 - shift
    e1, e2, dm = d.abs().mean(0), (d * d).mean(0), (mean64 - shift).abs()
    tm = K * e1 + U32 * mean64.abs()
    tv = K * (e2 + 2 * dm * e1)
    _report(f"{tag} mean", (stats[:, 0].double() - mean64).abs(), tm)
    var_k = stats[:, 1].double() ** -2 - EPS
    _report(f"{tag} var", (var_k - var64).abs(), tv + 8 * U32 * (var64 + EPS))
    unb = var64 * M / (M - 1) if M > 1 else var64
    scale = M / (M - 1) if M > 1 else 1.0
    rm64 = (1 - momentum) * shift + momentum * mean64
    rv64 = (1 - momentum) * rv0 + momentum * unb
    _report(f"{tag} running_mean", (rm_new.double() - rm64).abs(),
            momentum * tm + 4 * U32 * (shift.abs() + mean64.abs()))
    _report(f"{tag} running_var", (rv_new.double() - rv64).abs(),
            momentum * scale * tv + 4 * U32 * (rv0.abs() + unb.abs()))
    return mean64, var64


def _fwd_ref(x64, rp64, mean, invstd, gamma, beta, relu, res_mode):
    """(out64, E) of the fused forward; rp64 is r' (None without a residual)."""
    sc = invstd * gamma.double()
    sh = beta.double() - mean * sc
    xs = x64 * sc
    pre = xs + sh
    E = xs.abs() + sh.abs()
    if res_mode:
        E = E + rp64.abs()
    E = 4e-5 * E
    if res_mode == 2:
        pre = pre + rp64
    out = pre.clamp_min(0) if relu else pre
    if res_mode == 1:
        out = out + rp64
    return out, E


def _check_out(tag, y, out64, E):
    _report(f"{tag} out", (y.double() - out64).abs(), HALF * out64.abs() + (1 + HALF) * E)


def _check_mask(mk, y):
    assert torch.equal(mk, _pack_bits(y > 0)), "stored ReLU mask != (y > 0)"


def _check_fp8(q, amax_out, y, amax_prev):
    yf = y.float()
    # the kernel's scale, 448.f / amax_prev in fp32 (divided on the host: a correctly rounded fp32 division)
    qs = (torch.tensor(448.0) / torch.tensor(amax_prev, dtype=torch.float32)).item() if amax_prev > 0 else 1.0
    want = (yf * qs).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.view(torch.uint8).reshape(want.shape), want), "fp8 copy != float8_e4m3fn(clamp(y scale))"
    assert torch.equal(amax_out.view(torch.float32).reshape(()), yf.abs().max()), "amax_out != max|y|"


# ---------------------------------------------------------------------------------------------------------------
# drivers: raw launches through the C ABI (and the Python face of the parts entry point), outputs pre-filled
# ---------------------------------------------------------------------------------------------------------------
def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _run_fwd(entry, x, r, gamma, beta, rm, rv, relu, res_mode, mask=False, fp8=None, lazy=None, momentum=MOM):
    """One forward launch.  entry "fwd": dca_ops_bn_fwd (its own statistics pass); "parts": dca_ops_bn_fwd_parts
    through ops/functional.py _bn_fwd_parts, on partial sums the test built; "eval": dca_ops_bn_eval.  rm / rv are
    updated in place.  Returns dict(y, stats, mask, q, amax)."""
    N, F = _N(), _F()
    M, C = x.shape
    dev = x.device
    y = _nan_like(x)
    stats = torch.full((C, 2), float("nan"), dtype=torch.float32, device=dev)
    res = dict(y=y, stats=stats, mask=None, q=None, amax=None)
    if entry == "fwd":
        part = torch.empty((M + 255) // 256, C, 2, dtype=torch.float32, device=dev)
        N.check(N.lib().dca_ops_bn_fwd(N.ptr(x), N.ptr(r), N.ptr(y), N.ptr(part), N.ptr(stats), N.ptr(gamma),
                                       N.ptr(beta), N.ptr(rm), N.ptr(rv), M, C, EPS, momentum, int(relu),
                                       int(res_mode), N.ptr(F._ticket(dev, (C + 63) // 64)), N.stream(dev)), "bn_fwd")
    elif entry == "eval":
        N.check(N.lib().dca_ops_bn_eval(N.ptr(x), N.ptr(r), N.ptr(y), N.ptr(stats), N.ptr(gamma), N.ptr(beta),
                                        N.ptr(rm), N.ptr(rv), M, C, EPS, int(relu), int(res_mode), N.stream(dev)),
                "bn_eval")
    else:
        part, nparts = _parts128(x, rm)
        amax_prev = amax_out = None
        if mask:
            res["mask"] = torch.full((M * C // 8,), 0xFF, dtype=torch.uint8, device=dev)
        if fp8 is not None:
            res["q"] = torch.full((M, C), 0xFF, dtype=torch.uint8, device=dev)
            amax_prev = torch.tensor([fp8], dtype=torch.float32, device=dev)
            amax_out = res["amax"] = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
        F._bn_fwd_parts(x, r, y, part, nparts, stats, gamma, beta, rm, rv, EPS, momentum, relu, res_mode,
                        q=res["q"], amax_prev=amax_prev, amax_out=amax_out, mask=res["mask"], lazy_res=lazy)
    return res


def _run_bwd(dy, x, r, stats, gamma, beta, relu, res_mode, mask=None, want_dr=False, acc=None):
    """One dca_ops_bn_bwd.  acc: (g0, b0) to accumulate into (copies are made).  Returns dx, dr, dgamma, dbeta."""
    N, F = _N(), _F()
    M, C = x.shape
    dev = x.device
    dx = _nan_like(x)
    dr = _nan_like(x) if want_dr else None
    part = torch.empty((M + 255) // 256, C, 2, dtype=torch.float32, device=dev)
    sums = torch.full((C, 2), float("nan"), dtype=torch.float32, device=dev)
    if acc is not None:
        dgamma, dbeta = acc[0].clone(), acc[1].clone()
    else:
        dgamma = torch.full((C,), float("nan"), dtype=torch.float32, device=dev)
        dbeta = dgamma.clone()
    N.check(N.lib().dca_ops_bn_bwd(N.ptr(dy), N.ptr(x), N.ptr(r), N.ptr(stats), N.ptr(gamma), N.ptr(beta),
                                   N.ptr(part), N.ptr(sums), N.ptr(dgamma), N.ptr(dbeta), N.ptr(dx), N.ptr(dr), M, C,
                                   int(relu), int(res_mode), int(acc is not None), N.ptr(mask),
                                   N.ptr(F._ticket(dev, (C + 63) // 64)), N.stream(dev)), "bn_bwd")
    return dx, dr, dgamma, dbeta


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
# forward form: (entry, relu, res_mode, mask, fp8 amax_prev | None, on-the-fly residual BN)
FWD_SMALL = [("fwd", 0, 0, 0, None, 0), ("fwd", 1, 0, 0, None, 0), ("fwd", 1, 1, 0, None, 0),
             ("fwd", 1, 2, 0, None, 0),
             ("parts", 0, 0, 0, None, 0), ("parts", 1, 0, 0, None, 0), ("parts", 1, 1, 0, None, 0),
             ("parts", 1, 2, 0, None, 0), ("parts", 1, 2, 1, None, 0), ("parts", 1, 2, 1, 3.75, 0),
             ("parts", 1, 2, 1, 0.0, 0), ("parts", 1, 2, 0, None, 1), ("parts", 1, 2, 1, 3.75, 1),
             ("eval", 1, 2, 0, None, 0), ("eval", 0, 2, 0, None, 0)]
FWD_NT = [("fwd", 1, 0, 0, None, 0), ("fwd", 1, 1, 0, None, 0), ("parts", 1, 2, 1, None, 0),
          ("parts", 1, 2, 1, 3.75, 0), ("parts", 1, 2, 0, None, 1), ("eval", 1, 2, 0, None, 0)]
FWD_CACHED = [("parts", 1, 2, 0, None, 0)]
# backward form: (mode, relu, res_mode, mask, want_dr, accumulate)
BWD_SMALL = [(PLAIN, 0, 0, 0, 0, 0), (RELU, 1, 0, 0, 0, 0), (RELU, 1, 0, 0, 0, 1), (RELU, 1, 1, 0, 0, 0),
             (RES, 1, 2, 0, 1, 0), (MASK, 1, 2, 1, 1, 0), (MASK, 1, 2, 1, 1, 1), (MASK, 1, 2, 1, 0, 0),
             (MASK, 0, 0, 1, 0, 0), (MASK, 0, 0, 1, 1, 0)]
BWD_NT = [(PLAIN, 0, 0, 0, 0, 0), (RELU, 1, 0, 0, 0, 0), (RES, 1, 2, 0, 1, 0), (MASK, 1, 2, 1, 1, 0),
          (MASK, 1, 2, 1, 0, 1)]
BWD_CACHED = [(RELU, 1, 0, 0, 0, 0), (MASK, 1, 2, 1, 1, 0)]

SMALL_M = (1, 3, 127, 129, 255, 257, 1000)
SMALL_LANES = {8: 8, 72: 8, 128: 16, 384: 16}   # C -> channel lanes
# the smallest C % 128 == 0 shapes on each side of the two thresholds of bn_plan:
# (M, C) -> ((apply rows, nt), backward stats nt, (backward apply rows, nt))
EDGES = {((1 << 18) - 1, 128): ((256, 0), 0, (256, 0)),      # < 2^25 elements: 256 rows, cached
         ((1 << 18) + 77, 128): ((256, 0), 0, (128, 1)),     # >= 2^25: the 128-row backward apply
         ((1 << 19) - 1, 128): ((256, 0), 0, (128, 1)),      # < 2^26: still nothing else non-temporal
         ((1 << 19) + 77, 128): ((128, 1), 1, (128, 1)),     # >= 2^26: non-temporal everywhere, 128-row applies
         ((1 << 18) + 5, 256): ((128, 1), 1, (128, 1))}      # the same with two column groups
NT_SHAPES = [s for s, e in EDGES.items() if e[1]]


def _name(form):
    return "-".join("x" if v is None else str(v) for v in form)


def _cases(shapes, forms_of):
    return [pytest.param(M, C, f, id=f"{M}x{C}-{_name(f)}") for (M, C) in shapes for f in forms_of((M, C))]


SMALL_SHAPES = [(M, C) for C in SMALL_LANES for M in SMALL_M]


def _expect(M, C):
    """(lanes, apply, stats nt, backward apply) of a test shape, from the tables above."""
    if (M, C) in EDGES:
        return (16,) + EDGES[(M, C)]
    return SMALL_LANES[C], (256, 0), 0, (256, 0)


def _forward_case(dev, M, C, form):
    entry, relu, res_mode, mask, fp8, raff = form
    lanes, apply, snt, bapply = _expect(M, C)
    bwd_mode = -1 if (res_mode == 2 and not relu) else MASK if mask else (RES if res_mode == 2 else RELU) if relu \
        else PLAIN
    _assert_plan(M, C, relu, res_mode, mask, raff, lanes, apply, (bwd_mode, snt, bapply[0], bapply[1]))
    I = _inputs(M, C, str(dev))
    x, gamma, beta = I["x"], I["gamma"], I["beta"]
    r = I["r"] if res_mode else None
    x64 = x.double()
    rp64 = r.double() if res_mode else None
    zeros, ones = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    lazy = None
    if raff:  # the downsample branch: a statistics-only BN of r (no output), applied inside this pass
        rm_r, rv_r = zeros.clone(), ones.clone()
        rstats = torch.full((C, 2), float("nan"), dtype=torch.float32, device=dev)
        part, nparts = _parts128(r, zeros)
        _F()._bn_fwd_parts(r, None, None, part, nparts, rstats, I["rgamma"], I["rbeta"], rm_r, rv_r, EPS, MOM, False, 0)
        rmean, rvar = _check_stats("residual", rstats, rm_r, rv_r, rp64, zeros, ones)
        rsc = (rvar + EPS) ** -0.5 * I["rgamma"].double()
        rp64 = rp64 * rsc + (I["rbeta"].double() - rmean * rsc)
        lazy = (rstats, I["rgamma"], I["rbeta"])
    if entry == "eval":
        mean64, var64 = _stats64(x64)
        rm, rv = (mean64 * 0.9 + 0.05).float(), (var64 * 1.1).float()
        rm0, rv0 = rm.clone(), rv.clone()
        out64, E = _fwd_ref(x64, rp64, rm.double(), (rv.double() + EPS) ** -0.5, gamma, beta, relu, res_mode)
        res = _run_fwd("eval", x, r, gamma, beta, rm, rv, relu, res_mode)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
        _check_out("eval", res["y"], out64, E)
        return
    mean64, var64 = _stats64(x64)
    out64, E = _fwd_ref(x64, rp64, mean64, (var64 + EPS) ** -0.5, gamma, beta, relu, res_mode)
    del rp64
    rm, rv = zeros.clone(), ones.clone()
    for call in ("first", "second"):  # shift 0, then the previous batch's mean
        rm_old, rv_old = rm.clone(), rv.clone()
        res = _run_fwd(entry, x, r, gamma, beta, rm, rv, relu, res_mode, mask=mask, fp8=fp8, lazy=lazy)
        _check_stats(call, res["stats"], rm, rv, x64, rm_old, rv_old)
        _check_out(call, res["y"], out64, E)
        if mask:
            _check_mask(res["mask"], res["y"])
        if fp8 is not None:
            _check_fp8(res["q"], res["amax"], res["y"], fp8)
        rm.copy_(res["stats"][:, 0])


def _backward_case(dev, M, C, form):
    mode, relu, res_mode, mask, want_dr, acc = form
    lanes, apply, snt, bapply = _expect(M, C)
    _assert_plan(M, C, relu, res_mode, mask, 0, lanes, apply, (mode, snt, bapply[0], bapply[1]))
    I = _inputs(M, C, str(dev))
    x, dy, gamma, beta = I["x"], I["dy"], I["gamma"], I["beta"]
    x64, dy64, g64, b64 = x.double(), dy.double(), gamma.double(), beta.double()
    mean64, var64 = _stats64(x64)
    stats = torch.stack([mean64, (var64 + EPS) ** -0.5], 1).float().contiguous()
    mu, inv = stats[:, 0].double(), stats[:, 1].double()
    xh = (x64 - mu) * inv
    r = I["r"] if mode == RES else None
    if mode in (RELU, RES):
        sc = inv * g64
        sh = b64 - mu * sc
        pre = xh * g64 + b64
        # E, and the same bound in the backward's own form (xhat gamma + beta): the smaller of the two
        E = torch.minimum((x64 * sc).abs() + sh.abs(), (xh * g64).abs() + b64.abs())
        if mode == RES:
            pre = pre + r.double()
            E = E + r.double().abs()
        E = 4e-5 * E
        keep, A = pre > 0, pre.abs() <= E
        del pre, E
    else:
        keep = I["bits"] if mode == MASK else torch.ones_like(x, dtype=torch.bool)
        A = torch.zeros_like(keep)
    nA = int(A.sum())
    print(f"ambiguous {nA} of {A.numel()}")
    assert nA <= A_CAP * A.numel(), (nA, A.numel())
    dz = torch.where(keep, dy64, torch.zeros_like(dy64))
    ady = dy64.abs() * A
    sb, sg = dz.sum(0), (dz * xh).sum(0)
    tb = K * dz.abs().sum(0) + ady.sum(0)
    tg = K * (dz * xh).abs().sum(0) + (ady * xh.abs()).sum(0)
    del ady

    accv = (I["g0"], I["b0"]) if acc else None
    dx, dr, dgamma, dbeta = _run_bwd(dy, x, r, stats, gamma, beta, relu, res_mode, mask=I["mask"] if mask else None,
                                     want_dr=bool(want_dr), acc=accv)
    ref_g, ref_b = (sg + I["g0"].double(), sb + I["b0"].double()) if acc else (sg, sb)
    _report("dgamma", (dgamma.double() - ref_g).abs(), tg + (U32 * ref_g.abs() if acc else 0))
    _report("dbeta", (dbeta.double() - ref_b).abs(), tb + (U32 * ref_b.abs() if acc else 0))

    ca = g64 * inv
    cb = -ca * inv * sg / M
    cd = -ca * sb / M - cb * mu
    pushed = ca.abs() * (tb + xh.abs() * tg) / M
    fixed = (cb * x64).abs() + cd.abs()
    dxk = dx.double()

    def miss(dzv):  # error and bound of dx against the reference with this dz
        d64 = ca * (dzv - sb / M - xh * sg / M)
        return (dxk - d64).abs(), HALF * d64.abs() + pushed + 4 * ULP32 * ((ca * dzv).abs() + fixed)
    err, bound = miss(dz)
    if nA:  # the other branch, where the reference cannot tell
        dz2 = torch.where(A, torch.where(keep, torch.zeros_like(dy64), dy64), dz)
        err2, bound2 = miss(dz2)
        other = A & ~(err <= bound)
        err, bound = torch.where(other, err2, err), torch.where(other, bound2, bound)
    _report("dx", err, bound)
    if want_dr:
        zero = torch.zeros_like(dy)
        bits = dr.view(torch.int16)
        kept, dropped = bits == dy.view(torch.int16), bits == zero.view(torch.int16)
        ok = torch.where(A, kept | dropped, torch.where(keep, kept, dropped))
        assert bool(ok.all()), f"dr != bf16(dz) at {int((~ok).sum())} elements"
    else:
        assert dr is None


@pytest.mark.parametrize("M,C,form", _cases(SMALL_SHAPES, lambda s: FWD_SMALL))
def test_bn_forward_small(gpu, M, C, form):
    """Tail rows, clamped loads and partial channel blocks of the 8- and 16-lane kernels: every forward form, from
    both entry points and in eval mode, on M around the 128- / 256-row blocks and C below, at and above one block."""
    _forward_case(gpu, M, C, form)


@pytest.mark.parametrize("M,C,form", _cases(SMALL_SHAPES, lambda s: BWD_SMALL))
def test_bn_backward_small(gpu, M, C, form):
    """The four ways of recovering dz (with both legal mask uses, dr on and off, accumulate on and off) on the same
    small shapes."""
    _backward_case(gpu, M, C, form)


@pytest.mark.parametrize("M,C,form", _cases(EDGES, lambda s: FWD_NT if s in NT_SHAPES else FWD_CACHED))
def test_bn_forward_policy_edges(gpu, M, C, form):
    """The forward on both sides of bn_plan's thresholds: k_bn_apply<16, 128, true, *> (non-temporal, with and without
    the on-the-fly residual BN) on the two shapes of >= 2^26 elements, the cached 256-row form just below."""
    _forward_case(gpu, M, C, form)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M,C,form", _cases(EDGES, lambda s: BWD_NT if s in NT_SHAPES else BWD_CACHED))
def test_bn_backward_policy_edges(gpu, M, C, form):
    """The backward on both sides of the thresholds: non-temporal k_bn_bwd_stats and the 128-row non-temporal
    k_bn_bwd_apply in all four modes at >= 2^26 elements, the 128-row apply alone from 2^25, 256 rows below."""
    _backward_case(gpu, M, C, form)
    torch.cuda.empty_cache()


def test_bn_backward_face_omits_dr(gpu):
    """ops/functional.py _bn_backward with the stored mask and want_dr = False allocates and returns no dr, and its dx
    and sums are those of the raw call."""
    M, C = 257, 128
    I = _inputs(M, C, str(gpu))
    x64 = I["x"].double()
    mean64, var64 = _stats64(x64)
    stats = torch.stack([mean64, (var64 + EPS) ** -0.5], 1).float().contiguous()
    dx, dr, dgamma, dbeta = _F()._bn_backward(I["dy"], I["x"], None, I["gamma"], I["beta"], stats, True, 2,
                                              mask=I["mask"], want_dr=False)
    assert dr is None
    dx2, dr2, dgamma2, dbeta2 = _run_bwd(I["dy"], I["x"], None, stats, I["gamma"], I["beta"], 1, 2, mask=I["mask"])
    assert dr2 is None and torch.equal(dx.view(torch.int16), dx2.view(torch.int16))
    assert torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)
    _, dr3, _, _ = _F()._bn_backward(I["dy"], I["x"], None, I["gamma"], I["beta"], stats, True, 2, mask=I["mask"])
    assert torch.equal(dr3.view(torch.int16), torch.where(I["bits"], I["dy"], torch.zeros_like(I["dy"])).view(torch.int16))
