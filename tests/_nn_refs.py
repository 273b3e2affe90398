"""Plain float64 / integer references of the ops library's data-movement and head kernels (csrc/ops_nn.hip: im2col,
col2im, max pool, global average pool, cross-entropy, fp8 quantisation, the input layouts, the weight-pack gathers) and
of a convolution's input / weight gradient, with the case tables of tests/test_ops_nn_forms_gpu.py and
tests/test_ops_conv_dgrad_gpu.py.

tests/test_ops_nn_refs.py proves every reference here against an independent torch formulation on the CPU, and every
exactness precondition the GPU modules rely on, over the same tables -- so a GPU failure is the kernel's.  Activations are
channels-last ([N, H, W, C]) as the kernels see them; nothing here touches a GPU or imports the package."""
import math

import torch

F64 = torch.float64

# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
# (n, h, w, c, k, s, p)
IM2COL_GEOMS = [(2, 5, 7, 8, 3, 1, 1), (2, 6, 5, 16, 3, 2, 1), (2, 9, 7, 3, 3, 1, 1), (2, 7, 6, 12, 3, 2, 0),
                (2, 11, 9, 3, 7, 2, 3), (1, 4, 4, 5, 1, 2, 0), (2, 5, 5, 8, 5, 1, 2)]
COL2IM_GEOMS = IM2COL_GEOMS + [(2, 7, 5, 8, 3, 2, 1), (2, 6, 6, 8, 1, 2, 0)]
POOL_N = 2
# (k, s, p, h, w, c)
POOL_CASES = [(2, 2, 0, 6, 8, 8), (2, 2, 0, 7, 5, 5), (2, 2, 0, 7, 5, 24),
              (3, 2, 1, 8, 12, 8), (3, 2, 1, 6, 4, 24), (3, 2, 1, 8, 12, 24),
              (3, 2, 1, 7, 9, 8), (3, 2, 1, 7, 9, 5), (3, 2, 1, 8, 12, 5),
              (3, 1, 1, 5, 6, 24), (3, 1, 1, 5, 6, 5), (3, 3, 0, 7, 7, 8), (3, 3, 0, 7, 7, 5),
              (5, 2, 2, 9, 6, 8), (5, 2, 2, 9, 6, 5)]
POOL_RANDOM = [(3, 2, 1, 8, 12, 8), (3, 2, 1, 7, 9, 5)]   # one per family: randn x, random bf16 dy, NaN planting
POOL_VALUES = (-1.5, 0.0, 0.25, 2.0)                      # <= 4 distinct bf16 values: ties in most windows
AVG_SHAPES = [(2, 1, 8), (3, 49, 40), (2, 16, 5), (2, 4, 300)]   # (n, hw, c)
# (B, K, label mode): "ends" puts class 0 first and K - 1 last, "first" / "last" the one label of a single row,
# "clamp" also plants -1 and K (the kernel clamps them to 0 and K - 1)
CE_CASES = [(1, 1, "ends"), (1, 10, "first"), (1, 10, "last"), (33, 10, "ends"), (33, 10, "clamp"), (64, 63, "ends"),
            (65, 64, "ends"), (7, 65, "ends"), (7, 65, "clamp"), (200, 1000, "ends")]
CE_OFFSETS = (0.0, 80.0, -80.0, 1e4)
CE_T_MAX = 100.0
FP8_SIZES = [1, 3, 4, 1023, 4099]
# conv input / weight gradient: name -> ((n, h, w, ci, co, k, s, p), packed, route)
DGRAD_CASES = {
    "1x1_tb": ((2, 5, 7, 16, 24, 1, 1, 0), False, "1x1_tb"),
    "1x1_packed": ((2, 5, 7, 16, 24, 1, 1, 0), True, "1x1_packed"),
    "s1_fly_p1": ((2, 6, 5, 8, 16, 3, 1, 1), False, "s1_fly"),
    "s1_fly_p0": ((2, 7, 6, 8, 8, 3, 1, 0), False, "s1_fly"),
    "s1_fly_p2": ((2, 5, 5, 8, 8, 3, 1, 2), False, "s1_fly"),
    "s1_packed_p1": ((2, 6, 5, 8, 16, 3, 1, 1), True, "s1_packed"),
    "s1_packed_p0": ((2, 7, 6, 8, 8, 3, 1, 0), True, "s1_packed"),
    "s1_packed_p2": ((2, 5, 5, 8, 8, 3, 1, 2), True, "s1_packed"),
    "parity4": ((2, 8, 6, 8, 16, 3, 2, 1), True, "parity4"),
    "parity4_hw": ((2, 6, 10, 16, 8, 3, 2, 1), True, "parity4"),
    "parity1": ((2, 6, 8, 8, 16, 1, 2, 0), True, "parity1"),
    "col2im_odd_packed": ((2, 7, 5, 8, 8, 3, 2, 1), True, "col2im"),
    "col2im_s2_nopack": ((2, 8, 6, 8, 8, 3, 2, 1), False, "col2im"),
    # C = 3 at stride 1: _conv_bwd's stride-1 branch does not ask for C % 8 == 0, so this geometry takes the implicit
    # conv over flipped weights (3 output columns); the forward and the weight gradient run on the explicit cols
    "c3_s1": ((2, 6, 6, 3, 8, 3, 1, 1), False, "s1_fly"),
    "col2im_c3_s2": ((2, 6, 6, 3, 8, 3, 2, 1), False, "col2im"),   # the same at stride 2: the scalar k_col2im
    "col2im_k5": ((2, 8, 8, 8, 8, 5, 2, 2), True, "col2im"),
}
DGRAD_MASKED = {  # a deferred masked join source (GradJoin.defer_masked) meeting a 1x1 / a 3x3 consumer
    "masked_1x1_tb": ((2, 5, 7, 16, 24, 1, 1, 0), False, "1x1_tb"),
    "masked_1x1_packed": ((2, 5, 7, 16, 24, 1, 1, 0), True, "1x1_packed"),
    "unmask_3x3": ((2, 6, 5, 8, 16, 3, 1, 1), True, "s1_packed"),
}


def out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randint(g, lo, hi, shape):
    """Integers in [lo, hi] as float64."""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# im2col / col2im: column (kh KW + kw) C + c of row (n, oh, ow); columns K..Kp zero
# ---------------------------------------------------------------------------------------------------------------------
def im2col(x, k, s, p, kp=None):
    """x [N, H, W, C] (any dtype: pure movement) -> cols [N Ho Wo, Kp]."""
    n, h, w, c = x.shape
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    kk = k * k * c
    kp = (kk + 7) // 8 * 8 if kp is None else kp
    xp = x.new_zeros(n, h + 2 * p, w + 2 * p, c)
    xp[:, p:p + h, p:p + w] = x
    cols = x.new_zeros(n, ho, wo, kp)
    for a in range(k):
        for b in range(k):
            t = a * k + b
            cols[..., t * c:(t + 1) * c] = xp[:, a:a + s * (ho - 1) + 1:s, b:b + s * (wo - 1) + 1:s]
    return cols.view(n * ho * wo, kp)


def col2im(dcols, geom, dx_old=None):
    """dcols [N Ho Wo, Kp] float64 -> dx [N, H, W, C] float64 = the sum over the taps that read each pixel (+ dx_old);
    columns >= K are never read."""
    n, h, w, c, k, s, p = geom
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    d = dcols.view(n, ho, wo, -1)
    dxp = torch.zeros(n, h + 2 * p + s, w + 2 * p + s, c, dtype=F64)
    for a in range(k):
        for b in range(k):
            t = a * k + b
            dxp[:, a:a + s * (ho - 1) + 1:s, b:b + s * (wo - 1) + 1:s] += d[..., t * c:(t + 1) * c]
    dx = dxp[:, p:p + h, p:p + w].clone()
    return dx if dx_old is None else dx + dx_old


# ---------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------
def pool_family(k, s, p, h, w, c):
    """The kernel family csrc/ops_api.hip pool_k3s2 picks."""
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    return "k3s2" if (k == 3 and s == 2 and p == 1 and h == 2 * ho and w == 2 * wo and c % 8 == 0) else "generic"


def pool_input(case, random=False):
    """x [N, H, W, C] float64 of bf16 values: drawn from POOL_VALUES (the first three for a 2x2 window, so that most
    windows of every case hold a tie for the maximum), or randn."""
    k, s, p, h, w, c = case
    g = gen(sum(case))
    if random:
        return torch.randn(POOL_N, h, w, c, generator=g).to(torch.bfloat16).to(F64)
    vals = torch.tensor(POOL_VALUES[:3] if k == 2 else POOL_VALUES, dtype=F64)
    return vals[torch.randint(0, len(vals), (POOL_N, h, w, c), generator=g)]


def _windows(x, k, s, p, fill):
    n, h, w, c = x.shape
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    xp = torch.full((n, h + 2 * p + s, w + 2 * p + s, c), fill, dtype=x.dtype)
    xp[:, p:p + h, p:p + w] = x
    for a in range(k):
        for b in range(k):
            yield a * k + b, xp[:, a:a + s * (ho - 1) + 1:s, b:b + s * (wo - 1) + 1:s]


def maxpool_fwd(x, k, s, p):
    """x [N, H, W, C] float64 -> (y, tap uint8): tap = kh K + kw of the first maximum in ascending tap order over the
    taps inside the image; a NaN beats any number and the first NaN wins."""
    n, h, w, c = x.shape
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    best = torch.full((n, ho, wo, c), -math.inf, dtype=F64)
    tap = torch.zeros(n, ho, wo, c, dtype=torch.int64)
    valid_img = torch.ones(n, h, w, c, dtype=F64)
    for (t, v), (_, ok) in zip(_windows(x, k, s, p, 0.0), _windows(valid_img, k, s, p, 0.0)):
        take = (ok > 0) & ((v > best) | (torch.isnan(v) & ~torch.isnan(best)))
        best = torch.where(take, v, best)
        tap = torch.where(take, torch.full_like(tap, t), tap)
    return best, tap.to(torch.uint8)


def maxpool_bwd(dy, tap, geom, dtype=F64, reverse=False):
    """(dx, sum |terms|, smallest non-zero |term| (inf where none)) per input pixel, float64 (dtype / reverse: the
    same sums accumulated in another precision and tap order, for the exactness proof)."""
    n, h, w, c, k, s, p = geom
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    shape = (n, h + 2 * p + s, w + 2 * p + s, c)
    dy = dy.to(dtype)
    dxp, sab, mn = torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype), torch.full(shape, math.inf, dtype=dtype)
    order = range(k - 1, -1, -1) if reverse else range(k)
    for a in order:
        for b in order:
            sl = (slice(None), slice(a, a + s * (ho - 1) + 1, s), slice(b, b + s * (wo - 1) + 1, s))
            term = torch.where(tap == a * k + b, dy, torch.zeros_like(dy))
            dxp[sl] += term
            sab[sl] += term.abs()
            mn[sl] = torch.minimum(mn[sl], torch.where(term != 0, term.abs(), torch.full_like(term, math.inf)))
    crop = (slice(None), slice(p, p + h), slice(p, p + w))
    return dxp[crop].clone(), sab[crop].clone(), mn[crop].clone()


def fp32_sum_exact(sab, mn):
    """Where a sum of bf16 addends is exact in fp32 in any order: every addend is a multiple of q = 2^(e - 7), e the
    exponent of the smallest non-zero one, so is every partial sum, and each is at most sum|terms| in size; a multiple
    of q below 2^24 q is an fp32 number.  (No non-zero addend: the sum is 0.)"""
    e = torch.frexp(torch.where(torch.isinf(mn), torch.ones_like(mn), mn))[1] - 1
    q = torch.ldexp(torch.ones_like(mn), e - 7)
    return torch.isinf(mn) | (sab < q * 2.0 ** 24)


# ---------------------------------------------------------------------------------------------------------------------
# global average pool over x [N, HW, C]
# ---------------------------------------------------------------------------------------------------------------------
def avgpool_fwd(x):
    return x.to(F64).mean(1)


def avgpool_bwd(dy, hw):
    """dy [N, C] -> dx [N, HW, C] float64."""
    return (dy.to(F64) / hw)[:, None, :].expand(-1, hw, -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def ce_inputs(B, K, mode):
    """(logits fp32 [B, K], labels int64 [B]): 3 randn plus a per-row offset; row 1 (row 0 of a single row at K > 1 in
    mode "last") has one dominant logit, the others 60 below."""
    g = gen(7919 * B + K)
    x = 3.0 * torch.randn(B, K, generator=g, dtype=torch.float32)
    dom = 1 if B > 1 else (0 if mode == "last" and K > 1 else None)
    if dom is not None and K > 1:
        x[dom] -= 60.0
        x[dom, K // 2] += 60.0
    off = torch.tensor([CE_OFFSETS[b % 4] for b in range(B)], dtype=torch.float32)
    x = (x + off[:, None]).contiguous()
    y = torch.randint(0, K, (B,), generator=g)
    y[0] = K - 1 if mode == "last" else 0
    if B > 1:
        y[-1] = K - 1
    if mode == "clamp":
        y[2], y[3] = -1, K
    return x, y


def cross_entropy(logits, labels, grad_scale):
    """float64 (row losses [B], their mean, dlogits [B, K], lse [B], s [B] = sum exp(row - max), p [B, K]); labels
    clamped to [0, K - 1] as the kernel does."""
    x = logits.to(F64)
    B, K = x.shape
    y = labels.clamp(0, K - 1)
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    lse = (m + torch.log(s)).squeeze(1)
    loss = lse - x.gather(1, y[:, None]).squeeze(1)
    p = e / s
    onehot = torch.zeros_like(p).scatter_(1, y[:, None], 1.0)
    return loss, loss.mean(), (p - onehot) * float(grad_scale), lse, s.squeeze(1), p


# ---------------------------------------------------------------------------------------------------------------------
# fp8 e4m3 (OCP e4m3fn: bias 7, no infinities, largest finite 448)
# ---------------------------------------------------------------------------------------------------------------------
def e4m3_encode(v):
    """float64 |v| <= 448 -> e4m3fn byte, round to nearest even, written out in integer steps."""
    a = v.abs()
    e = (torch.frexp(torch.where(a > 0, a, torch.ones_like(a)))[1] - 1).clamp_min(-6)
    m = torch.round(torch.ldexp(a, 3 - e))                 # in units of 2^(e - 3); torch.round is half-to-even
    up = m >= 16                                            # rounded up into the next binade
    e, m = torch.where(up, e + 1, e), torch.where(up, m / 2, m)
    bits = torch.where(m < 8, m, (e + 7).to(F64) * 8 + (m - 8)).to(torch.int64)   # m < 8: subnormal (e = -6) or zero
    return (bits | (torch.signbit(v).to(torch.int64) << 7)).to(torch.uint8)


def quant_fp8(x):
    """x fp32 / bf16 -> (amax bits int32, q uint8) as k_amax / k_quant_fp8 compute them: amax = max |x| (exact),
    sc = float32(448) / float32(amax) in fp32 (1 for amax == 0), q = e4m3(clamp(fp32(x) sc, +-448))."""
    xf = x.float().reshape(-1)
    amax = xf.abs().max()
    sc = torch.tensor(448.0, dtype=torch.float32) / amax if amax > 0 else torch.tensor(1.0)
    v = (xf * sc).clamp(-448.0, 448.0)
    return int(amax.view(torch.int32)), v.to(torch.float8_e4m3fn).view(torch.uint8).view(x.shape)


FP8_KINDS = ("randn", "zero", "pow2_up", "pow2_down")


def fp8_input(n, kind):
    """fp32 values exact in bf16.  pow2_*: amax = 448 2^k (k = 3 / -5), so the scale 448 / amax is a power of two and
    x sc is exact whatever the division does; the values then cover every e4m3 binade, ties included."""
    g = gen(31 * n + len(kind))
    if kind == "zero":
        return torch.zeros(n)
    x = (torch.randn(n, generator=g) * 3.0).to(torch.bfloat16).float()
    if kind.startswith("pow2"):
        top = 448.0 * (8.0 if kind == "pow2_up" else 2.0 ** -5)
        x = (torch.randn(n, generator=g) * top / 3).clamp(-top, top)
        x = x * torch.ldexp(torch.ones(n), -torch.randint(0, 12, (n,), generator=g))   # reach the subnormal binades
        x = x.to(torch.bfloat16).float()
        x[n // 2] = -top
    return x


def fp8_alpha(amax_a, amax_b, extra):
    """fp32 tensors -> fp32, in k_fp8_alpha's order."""
    f = torch.float32
    one, d = torch.tensor(1.0, dtype=f), torch.tensor(448.0, dtype=f)
    a = amax_a / d if amax_a > 0 else one
    b = amax_b / d if amax_b > 0 else one
    return a * b * torch.tensor(extra, dtype=f)


# ---------------------------------------------------------------------------------------------------------------------
# input layouts
# ---------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc8(x):
    """x [N, C, H, W] fp32 -> [N, H, W, 8] bf16: y[n][p][c] = bf16(x[n][c][p]), channels C..7 zero."""
    n, c, h, w = x.shape
    y = torch.zeros(n, h, w, 8, dtype=torch.bfloat16)
    for ch in range(c):
        y[..., ch] = x[:, ch].to(torch.bfloat16)
    return y


def nchw_to_s2d16(x, hs, ws, P):
    """y[n][Y][X][(2 ph + pw) C + c] = x[n][c][2Y + ph - P][2X + pw - P], zero outside the image and for channels
    4C..15 (the index formula of k_nchw_to_s2d16's comment)."""
    n, c, h, w = x.shape
    y = torch.zeros(n, hs, ws, 16, dtype=torch.bfloat16)
    for Y in range(hs):
        for X in range(ws):
            for ph in (0, 1):
                for pw in (0, 1):
                    r, q = 2 * Y + ph - P, 2 * X + pw - P
                    if 0 <= r < h and 0 <= q < w:
                        y[:, Y, X, (2 * ph + pw) * c:(2 * ph + pw) * c + c] = x[:, :, r, q].to(torch.bfloat16)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# convolution gradients
# ---------------------------------------------------------------------------------------------------------------------
def parity_classes(w, p):
    """WeightPack._parity_classes' docstring, spelled out with loops: input pixels of parity (ph, pw) of a stride-2
    conv receive dY through the taps kh with (ph + p - kh) even, from dY row i + (ph + p - kh) / 2; taps ordered by that
    offset, pad = -(smallest offset); matrix [Cin][(a_h KWc + a_w) Cout + co] = w[co][ci][kh_a][kw_a].
    Returns {(ph, pw): (kh list, kw list, (pad_h, pad_w), matrix float64)} for the classes that have taps."""
    co, ci, k, _ = w.shape

    def taps(par):
        t = sorted(((par + p - kk) // 2, kk) for kk in range(k) if (par + p - kk) % 2 == 0)
        return ([kk for _, kk in t], -t[0][0]) if t else ([], 0)

    out = {}
    for ph in (0, 1):
        for pw in (0, 1):
            (khl, pad_h), (kwl, pad_w) = taps(ph), taps(pw)
            if not khl or not kwl:
                continue
            m = torch.zeros(ci, len(khl) * len(kwl) * co, dtype=F64)
            for ah, kh in enumerate(khl):
                for aw, kw in enumerate(kwl):
                    col = (ah * len(kwl) + aw) * co
                    m[:, col:col + co] = w[:, :, kh, kw].to(F64).t()
            out[(ph, pw)] = (khl, kwl, (pad_h, pad_w), m)
    return out


def parity_dgrad(dy, w, p, h, wd):
    """dx [N, H, W, Cin] float64 of a stride-2 conv assembled from its parity classes as _conv_bwd runs them: class
    (ph, pw) is a stride-1 conv over dY [N, Ho, Wo, Cout] with its matrix, zero outside dY, written to the pixels
    (2i + ph, 2j + pw), i < (H - ph + 1) // 2, j < (W - pw + 1) // 2; pixels of a class without taps stay zero."""
    n, ho, wo, co = dy.shape
    ci = w.shape[1]
    dx = torch.zeros(n, h, wd, ci, dtype=F64)
    for (ph, pw), (khl, kwl, (pad_h, pad_w), m) in parity_classes(w, p).items():
        hc, wc = (h - ph + 1) // 2, (wd - pw + 1) // 2
        big = 8
        dyp = torch.zeros(n, hc + 2 * big, wc + 2 * big, co, dtype=F64)
        dyp[:, big:big + ho, big:big + wo] = dy
        acc = torch.zeros(n, hc, wc, ci, dtype=F64)
        for ah in range(len(khl)):
            for aw in range(len(kwl)):
                col = (ah * len(kwl) + aw) * co
                win = dyp[:, big + ah - pad_h:big + ah - pad_h + hc, big + aw - pad_w:big + aw - pad_w + wc]
                acc += win @ m[:, col:col + co].t()
        dx[:, ph::2, pw::2] = acc
    return dx


def conv_dgrad(dy, w, s, p, h, wd):
    """dy [N, Ho, Wo, Cout], w [Cout, Cin, K, K] -> dx [N, H, W, Cin] float64 (conv_transpose2d)."""
    k = w.shape[2]
    ho, wo = dy.shape[1], dy.shape[2]
    oph, opw = h - ((ho - 1) * s - 2 * p + k), wd - ((wo - 1) * s - 2 * p + k)
    dx = torch.nn.functional.conv_transpose2d(dy.to(F64).permute(0, 3, 1, 2), w.to(F64), stride=s, padding=p,
                                              output_padding=(oph, opw))
    return dx.permute(0, 2, 3, 1).contiguous()


def conv_wgrad(x, dy, k, s, p):
    """x [N, H, W, Cin], dy [N, Ho, Wo, Cout] -> dw [Cout, Cin, K, K] float64 = dY^T . im2col(x)."""
    c = x.shape[3]
    cols = im2col(x.to(F64), k, s, p, kp=k * k * c)
    dw = dy.to(F64).reshape(-1, dy.shape[3]).t() @ cols            # [Cout, (kh K + kw) C + c]
    return dw.view(-1, k, k, c).permute(0, 3, 1, 2).contiguous()


def weight_matrix(w):
    """[Cout, Cin, KH, KW] -> [Cout, K] with column (kh KW + kw) Cin + ci (the forward / col2im operand)."""
    return w.to(F64).permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def dgrad_inputs(geom, seed=0):
    """Integer operands: x bf16 in [-3, 3], w fp32 in [-2, 2], dy bf16 in [-3, 3], a join seed in [-8, 8], mask bits."""
    n, h, w_, ci, co, k, s, p = geom
    g = gen(1000 * sum(geom) + k + seed)
    ho, wo = out_size(h, k, s, p), out_size(w_, k, s, p)
    return dict(x=randint(g, -3, 3, (n, h, w_, ci)), w=randint(g, -2, 2, (co, ci, k, k)),
                dy=randint(g, -3, 3, (n, ho, wo, co)), seed=randint(g, -8, 8, (n, h, w_, ci)),
                sink=randint(g, -8, 8, (co, ci, k, k)),
                bits=torch.randint(0, 2, (n, h, w_, ci), generator=g).to(F64))


def pack_bits(bits):
    """[..] 0 / 1 -> bytes, bit j of byte e / 8 = element e = 8 (e / 8) + j."""
    wgt = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int64)
    return (bits.reshape(-1, 8).to(torch.int64) * wgt).sum(1).to(torch.uint8).contiguous()
