"""Plain CPU statement of the fp16x3 engine's number format (include/vqwave.h "The fp16x3 engine"), shared by
test_x3_ref_cpu.py and test_x3_range_gpu.py.  numpy only; everything that computes does so in float64, everything that
describes device memory returns the exact uint16 image.  Written from the header's sentences, not from the kernels' index
arithmetic: an operand x is held as two fp16 planes h1 = fp16(s x), h2 = fp16(s x - h1) of ONE power-of-two scale s per
tensor, planes are [plane][chunk of 8 channels][row][8], and a product is a1 b1 + a1 b2 + a2 b1 over s_a s_b.  VQW_X3_BF16: ONE
plane bf16(s x), rounded to nearest even, and one product a b (exact in fp32) -- bf16_round, contract_bf16, conv_bf16, wgrad_bf16."""
import math

import numpy as np

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
X3_BF16, X3_HALF_BLOCKS, X3_S2D = 1, 2, 4


def scaled(x, scale=1.0, scale_dev=1.0):
    """scale * scale_dev * x as the header orders it: the two scales meet in fp32 first, then one fp32 product per element."""
    sc = np.float32(np.float32(scale) * np.float32(scale_dev))
    with np.errstate(over='ignore', under='ignore'):
        return (np.asarray(x, np.float32) * sc).astype(np.float32)


def split(x32, flush=False):
    """(h1, h2) as float16: h1 = float16(x), h2 = float16(x - float32(h1)), both rounded to nearest even.
    flush: fp16 subnormals of both planes become zero (a matrix pipe that does not keep them)."""
    x32 = np.asarray(x32, np.float32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        h1 = x32.astype(np.float16)
        h2 = (x32 - h1.astype(np.float32)).astype(np.float16)
    if flush:
        h1 = np.where(np.abs(h1) < F16_MIN_NORMAL, np.float16(0), h1)
        h2 = np.where(np.abs(h2) < F16_MIN_NORMAL, np.float16(0), h2)
    return h1, h2


def bf16_bits(x32):
    """uint16 image of bf16(x), round to nearest even (finite x)."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x32):
    """float64 value of bf16(x): the 16 bits of bf16_bits(x) are the upper half of a float32."""
    return (bf16_bits(x32).astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(np.shape(x32))


def plane_bits(x32, bf16=False):
    """[planes] + x.shape uint16: the two fp16 pieces, or the single bf16 piece."""
    if bf16:
        return bf16_bits(x32)[None]
    h1, h2 = split(x32)
    return np.stack([h1.view(np.uint16), h2.view(np.uint16)])


def _rows_to_planes(p, out, kc0=0):
    """p [planes][rows][K] (K = 8 * chunks) -> out[plane][kc0 + chunk][row][8]."""
    P, rows, Kd = p.shape
    out[:P, kc0:kc0 + Kd // 8] = p.reshape(P, rows, Kd // 8, 8).transpose(0, 2, 1, 3)
    return out


def act_planes(x, scale=1.0, scale_dev=1.0, kc0=0, KC=0, mode=0, into=None):
    """vqw_f16x3_split_activations: x [B][C][T] fp32 -> [planes][KC][B*T][8] uint16, this tensor's C/8 chunks from chunk kc0
    (KC = 0: exactly C/8).  VQW_X3_S2D: [planes][2 C/8][B*T/2][8], sample t = 2 t' + r in chunk block r, row b T/2 + t'.
    into: the image the buffer held before (chunks outside the range keep it)."""
    B, C, T = x.shape
    bf = bool(mode & X3_BF16)
    p = plane_bits(scaled(x, scale, scale_dev), bf)                      # [P][B][C][T]
    P = p.shape[0]
    if mode & X3_S2D:
        out = np.zeros((P, 2 * C // 8, B * T // 2, 8), np.uint16) if into is None else into.copy()
        for r in (0, 1):
            rows = p[:, :, :, r::2].transpose(0, 1, 3, 2).reshape(P, B * T // 2, C)
            _rows_to_planes(rows, out, r * (C // 8))
        return out
    KC = KC if KC > 0 else C // 8
    out = np.zeros((P, KC, B * T, 8), np.uint16) if into is None else into.copy()
    return _rows_to_planes(p.transpose(0, 1, 3, 2).reshape(P, B * T, C), out, kc0)


def pack_weights(w, K, M, scale=1.0, scale_dev=1.0, mode=0):
    """vqw_f16x3_pack_weights: w [count][K][ldw] fp32 (row k, column m < M) -> [count][planes][K/8][M][8] uint16."""
    w = np.asarray(w, np.float32)
    w = w.reshape((-1,) + w.shape[-2:])[:, :K, :M]
    p = plane_bits(scaled(w, scale, scale_dev), bool(mode & X3_BF16))   # [P][count][K][M]
    P, cnt = p.shape[:2]
    out = np.zeros((cnt, P, K // 8, M, 8), np.uint16)
    for i in range(cnt):
        _rows_to_planes(p[:, i].transpose(0, 2, 1), out[i])
    return out


def transposed_matrix(src, K, M, k_inner, ld_src, blk_stride, count=1):
    """The matrices W'[i][k][m] = src[i * (K / k_inner) * blk_stride + (k // k_inner) * blk_stride + m * ld_src + k % k_inner]."""
    src = np.asarray(src, np.float32).reshape(-1)
    i = np.arange(count)[:, None, None] * (K // k_inner) * blk_stride
    k = np.arange(K)[None, :, None]
    m = np.arange(M)[None, None, :]
    return src[i + (k // k_inner) * blk_stride + m * ld_src + k % k_inner]


def pack_weights_t(src, K, M, k_inner, ld_src, blk_stride, scale=1.0, count=1, scale_dev=1.0, mode=0):
    """vqw_f16x3_pack_weights_t: the planes of pack_weights for the matrix stored transposed block by block."""
    return pack_weights(transposed_matrix(src, K, M, k_inner, ld_src, blk_stride, count), K, M, scale, scale_dev, mode)


def gate_row_order(R, mode=0):
    """Column of w (filter 0..R-1, gate R..2R-1) held by plane row m': blocks of hb rows (256, or 128 with
    VQW_X3_HALF_BLOCKS), each hb/2 filter channels followed by the hb/2 matching gate channels."""
    hb = 128 if mode & X3_HALF_BLOCKS else 256
    hh = hb // 2
    mp = np.arange(2 * R)
    blk, i = mp // hb, mp % hb
    return np.where(i < hh, hh * blk + i, R + hh * blk + i - hh)


def pack_gate_weights(w, ks, R, scale=1.0, scale_dev=1.0, mode=0):
    """vqw_f16x3_pack_gate_weights: w [count][ks][R][ldw] -> [count][planes][ks*R/8][2R][8], rows in block order."""
    w = np.asarray(w, np.float32)
    w = w.reshape((-1, ks * R, w.shape[-1]))[:, :, gate_row_order(R, mode)]
    return pack_weights(w, ks * R, 2 * R, scale, scale_dev, mode)


def contract(a, b, sa=1.0, sb=1.0, flush=False):
    """The engine's product of a [M][K] and b [K][N] (fp32): both operands scaled and split, the three terms
    a1 b1 + a1 b2 + a2 b1 summed in float64, divided by sa * sb.  The best any implementation of the format can do."""
    a1, a2 = (h.astype(np.float64) for h in split(scaled(a, sa), flush))
    b1, b2 = (h.astype(np.float64) for h in split(scaled(b, sb), flush))
    return (a1 @ b1 + a1 @ b2 + a2 @ b1) / (float(np.float32(sa)) * float(np.float32(sb)))


def planes_of(a, s, split_=split):
    """The two planes of s * a as float64 (split_: what stands in for split, e.g. an evaluation without the split)."""
    h1, h2 = split_(scaled(a, s))
    return np.asarray(h1, np.float64), np.asarray(h2, np.float64)


def three_terms(a1, a2, w1, w2, no_h2h1=False):
    """(sum, sum of absolute values) of a1 w1 + a1 w2 + a2 w1 over K: a [B][K][N], w [K][M] -> [B][M][N].
    no_h2h1: the a2 w1 term is left out (a deliberately wrong evaluation)."""
    mm = lambda w, a: np.matmul(w.T[None], a)  # noqa: E731
    val, ab = mm(w1 + w2, a1), mm(np.abs(w1) + np.abs(w2), np.abs(a1))
    if not no_h2h1:
        val, ab = val + mm(w1, a2), ab + mm(np.abs(w1), np.abs(a2))
    return val, ab


def gather(x, idx, leak=False):
    """x [B][C][L] read at idx [N] of every batch row -> [B][C][N]; outside [0, L) zero.  leak: the batch rows are one flat
    (batch, time) axis and only its two ends read zero -- the neighbouring batch row is read instead."""
    B, C, L = x.shape
    idx = np.asarray(idx)
    if not leak:
        ok = (idx >= 0) & (idx < L)
        return x[:, :, np.clip(idx, 0, L - 1)] * ok
    flat = x.transpose(1, 0, 2).reshape(C, B * L)
    f = (np.arange(B) * L)[:, None] + idx[None, :]
    ok = (f >= 0) & (f < B * L)
    return (flat[:, np.clip(f, 0, B * L - 1)] * ok).transpose(1, 0, 2)


def contract_bf16(a, b, sa=1.0, sb=1.0):
    """The bf16 engine's product of a [M][K] and b [K][N] (fp32): both operands scaled as in the fp16 path, each rounded to its
    ONE bf16 plane, multiplied in float64 (a bf16 x bf16 product is exact in fp32, so only the summation is left to the device),
    divided by sa * sb."""
    return (bf16_round(scaled(a, sa)) @ bf16_round(scaled(b, sb))) / (float(np.float32(sa)) * float(np.float32(sb)))


def bf16_truncate(x32):
    """float64 value of x with the lower 16 bits of its float32 image dropped: what a conversion that forgets to round gives."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return u.view(np.float32).astype(np.float64).reshape(np.shape(x32))


def unrounded(x32):
    """float64 value of x itself: an operand that never went through bf16."""
    return np.asarray(x32, np.float32).astype(np.float64)


def shifted(x, sh, leak=False):
    """x [B][C][T] read at t + sh (sh <= 0, -sh < T), zero before the start of the batch row.  leak: the check is missing -- the
    flat (batch, time) rows before the batch row are read instead (the previous batch row's end; nothing lies before batch 0)."""
    B, C, T = x.shape
    if sh == 0:
        return x.copy()
    assert -T < sh < 0
    out = np.zeros_like(x)
    out[:, :, -sh:] = x[:, :, :T + sh]
    if leak:
        out[1:, :, :-sh] = x[:-1, :, T + sh:]
    return out


def conv_bf16(x, w, taps, sx=1.0, sw=1.0, rnd=bf16_round, leak_tap=None):
    """Causal dilated conv on the bf16 engine, float64 sums: out[b][m][t] = sum_j sum_c rnd(sx x)[b][c][t + taps[j]] rnd(sw w)[j][c][m]
    / (sx sw); x [B][C][T], w [taps][C][M].  rnd / leak_tap build the deliberately wrong evaluations of test_x3_ref_cpu.py."""
    xr, wr = rnd(scaled(x, sx)), rnd(scaled(w, sw))
    out = 0.0
    for j, sh in enumerate(taps):
        out = out + np.einsum('bct,cm->bmt', shifted(xr, sh, leak=(j == leak_tap)), wr[j], optimize=True)
    return out / (float(np.float32(sx)) * float(np.float32(sw)))


def wgrad_bf16(p, q, taps, sp=1.0, sq=1.0, rnd=bf16_round, leak_tap=None):
    """Weight gradient on the bf16 engine, float64 sums: dw[j][c][o] = sum_{b,t} rnd(sp p)[b][c][t + taps[j]] rnd(sq q)[b][o][t] / (sp sq)."""
    pr, qr = rnd(scaled(p, sp)), rnd(scaled(q, sq))
    dw = np.stack([np.einsum('bct,bot->co', shifted(pr, sh, leak=(j == leak_tap)), qr, optimize=True) for j, sh in enumerate(taps)])
    return dw / (float(np.float32(sp)) * float(np.float32(sq)))


def gate_case(B, T, R, ks, d):
    """Inputs of the bf16 gate-conv tests (test_bf16_kernels_gpu.py, and the discrimination tests of test_x3_ref_cpu.py):
    x [B][R][T], w [ks][R][2R], bias [2R], cond [B][2R][cond_T] with cond_T = T / 64 (T / 32 where 64 does not divide T)."""
    rng = np.random.RandomState(1000 + d + T)
    cond_T = T // 64 if T % 64 == 0 else T // 32
    x = rng.standard_normal((B, R, T)).astype(np.float32)
    w = (rng.standard_normal((ks, R, 2 * R)) * 0.05).astype(np.float32)
    bias = (rng.standard_normal(2 * R) * 0.3).astype(np.float32)
    cond = (rng.standard_normal((B, 2 * R, cond_T)) * 0.3).astype(np.float32)
    return x, w, bias, cond


def gate_outputs(pre, bias, cond, T):
    """(tanh(f) * sigmoid(g), tanh(f), sigmoid(g)) of the float64 pre-activation [B][2R][T] + bias + the condition held for
    T / cond_T steps per frame; filter rows first, then the gate rows."""
    R = pre.shape[1] // 2
    pre = pre + bias.astype(np.float64)[None, :, None] + np.repeat(cond.astype(np.float64), T // cond.shape[2], axis=2)
    th, sg = np.tanh(pre[:, :R]), 1.0 / (1.0 + np.exp(-pre[:, R:]))
    return th * sg, th, sg


def wgrad_case(B, T, d, Q1, scaled_, Cp=256, Q0=512, ks=3):
    """Inputs of the bf16 weight-gradient tests: p [B][Cp][T], q = [q0; q1] [B][Q0 + Q1][T], the dw [ks][Cp][Q0 + Q1] accumulated
    into, the power-of-two guard scales (p, q0, q1); scaled_: gradients of 1e-6 lifted by 2^30 / 2^28."""
    rng = np.random.RandomState(100 + d)
    p = rng.standard_normal((B, Cp, T)).astype(np.float32)
    q0 = (rng.standard_normal((B, Q0, T)) * (1e-6 if scaled_ else 1.0)).astype(np.float32)
    q1 = (rng.standard_normal((B, Q1, T)) * (3e-6 if scaled_ else 1.0)).astype(np.float32)
    dw0 = rng.standard_normal((ks, Cp, Q0 + Q1)).astype(np.float32)
    sc = np.float32([4.0, 2.0 ** 30, 2.0 ** 28] if scaled_ else [1.0, 1.0, 1.0])
    return p, q0, q1, dw0, sc


def row_rel_l2(got, want, axis=-1):
    """Relative L2 error over `axis` of every row of `got` against `want`, in float64."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    num = np.sqrt(((got - want) ** 2).sum(axis))
    den = np.sqrt((want ** 2).sum(axis))
    return num / np.maximum(den, 1e-300)


def amax_bits(x):
    """Bit pattern (uint32) of max |x| over an fp32 array."""
    return int(np.abs(np.asarray(x, np.float32)).max().astype(np.float32).view(np.uint32))


def exponent_sweep():
    """amax bit patterns: every fp32 exponent field 0..254 with the smallest, the largest and a middle mantissa."""
    bits = []
    for e in range(255):
        for m in (0, 1, 0x2aaaaa, 0x7fffff):
            if e or m:
                bits.append((e << 23) | m)
    return np.array(bits, np.uint32)


SCALE_EXP_CLAMP = 100       # vqwave.h: the exponent of a scale is held to [-100, 100]


def update_scales(amax, scale, target_exp):
    """vqw_f16x3_update_scales on host arrays: amax uint32 bit patterns, scale float32.  Returns (new scale, flag).
    scale = 2^k with amax * scale in [2^(target_exp-1), 2^target_exp), k held to [-100, 100]; amax == 0 keeps the scale
    (a scale of 0 becomes 1); a non-finite amax raises the flag and keeps the scale."""
    amax = np.asarray(amax, np.uint32)
    out = np.array(scale, np.float32).copy()
    flag = 0
    for i, bits in enumerate(amax.tolist()):
        f = float(np.array(bits, np.uint32).view(np.float32))
        if not math.isfinite(f):
            flag = 1
        elif f == 0.0:
            if out[i] == 0.0:
                out[i] = 1.0
        else:
            _, e = math.frexp(f)                      # f = m 2^e, 0.5 <= m < 1: floor(log2 f) = e - 1
            k = max(-SCALE_EXP_CLAMP, min(SCALE_EXP_CLAMP, target_exp - e))
            out[i] = np.float32(math.ldexp(1.0, k))
    return out, flag
