"""Independent reference of the photometric term's record-slot path (plain helper module, in the style of tests/icp_rows_ref.py).

The oracle (oracle/orc_track.c: orc_rgb_residual, orc_rgb_step) and the kernels (csrc/track_reduce.hip: rgb_residual_body<true>,
csrc/track_rgb_step_dev.h) share one specification of the RGB step's sums,

    sums[k(i, j)] += RNE(clamp(row_i) * clamp(row_j) * 2^F)      clamp at +-2^((50 - F) / 2), wrapping 64-bit integers,

with F = rgb_fix_bits(sigma), and both implement it with the same floating-point trick.  Nothing of the oracle is called here: the
per-pixel residual (RGBResidual::getProducts, reduce.cu:785-865, its pose-dependent half: rgb_residual_pixel) and the Jacobian row
(RGBReduction::getProducts, reduce.cu:521-604: rgb_step_row) are stated in numpy f32 in the operation order of the kernels, sigma and F
from their integer rules, and the sums with Python's unbounded integers and exact rationals -- round(Fraction) is round-half-even by
definition, nothing is scaled or split; the 64-bit wrap is applied once at the end.

DOMAIN of the reference (every case of tests/rgb_cases.py keeps it; tests/test_cpu_rgb_cases.py asserts it):
  * cloud z is finite and > 0 wherever a record can point (production: g is gated by lastDepth > 0, and the cloud is its projection);
  * rows are finite, and no row entry or intermediate of a row is subnormal;
  * a planted stale slot count is <= the slot's capacity and a planted stale record holds in-range indices, so that a kernel which
    wrongly reads one produces wrong sums, never an out-of-range access or a long loop.

THE RECORD FORMAT, as a contract: a record is two 32-bit words, x = k (flat index of the pixel in the next image, where dIdx / dIdy are
read), y = g | (diff + 256) << 22 (g: flat index in the last image, where the cloud is read; diff = next - last intensity, an integer
in [-255, 255], so the field holds 1 .. 511).  Slot s of a launch with T threads per workgroup holds the records of the pixels
[s * 4T, (s + 1) * 4T) in any order, from record s * 4T on; slot_counts[s] is their number.  A culled tracker's residual pass visits the
slots first .. last only, first = (~lo_inv) >> sh, last = min((hi_p1 - 1) >> sh, n_slots - 1) with sh = log2(4T) - 8 (lo_inv / hi_p1
count 256-pixel chunks); hi_p1 == 0 is the empty range.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from icp_rows_ref import _f2i_rn

F32 = np.float32
FLT_EPSILON = F32(1.19209290e-07)
_M32, _M64 = 1 << 32, 1 << 64


def wrap32(v):
    """a Python integer as the C `int` that holds its low 32 bits"""
    return (int(v) + (1 << 31)) % _M32 - (1 << 31)


def wrap64(v):
    return (int(v) + (1 << 63)) % _M64 - (1 << 63)


# ------------------------------------------------------------------------------------------------ residual
def residual(c):
    """the pose-dependent half of RGBResidual::getProducts for EVERY pixel k of case `c` (the candidate mask is applied by the caller)
    -> ok bool [N], g int64 [N] (0 where not ok), diff int64 [N], and u0, v0 before rounding (f32) for the tie counts"""
    cols, rows = c.cols, c.rows
    k = np.arange(cols * rows)
    y = (k // cols).astype(np.int32); x = (k - y * cols).astype(np.int32)
    xf, yf = x.astype(F32), y.astype(F32)
    krk = np.asarray(c.krk, F32).reshape(9); kt = np.asarray(c.kt, F32).reshape(3)
    d1 = np.asarray(c.next_depth, F32).reshape(-1)
    with np.errstate(all="ignore"):
        td1 = d1 * (krk[6] * xf + krk[7] * yf + krk[8]) + kt[2]
        uq = (d1 * (krk[0] * xf + krk[1] * yf + krk[2]) + kt[0]) / td1
        vq = (d1 * (krk[3] * xf + krk[4] * yf + krk[5]) + kt[1]) / td1
        assert td1.dtype == F32 and uq.dtype == F32
        u0, v0 = _f2i_rn(uq), _f2i_rn(vq)
        inb = (u0 >= 0) & (v0 >= 0) & (u0 < cols) & (v0 < rows)
        g = np.where(inb, v0 * cols + u0, 0)
        d0 = np.asarray(c.last_depth, F32).reshape(-1)[g]
        li = np.asarray(c.last_image, np.uint8).reshape(-1)[g]
        ok = inb & (d0 > 0) & (np.abs(td1 - d0) <= F32(c.max_dd)) & (li != 0)
    diff = np.asarray(c.next_image, np.uint8).reshape(-1).astype(np.int64) - li.astype(np.int64)
    return dict(ok=ok, inb=inb, g=np.where(ok, g, 0), diff=np.where(ok, diff, 0), uq=uq, vq=vq, td1=td1, d0=d0, li=li)


def slot_range(c, threads):
    """(first, last) slot the residual pass visits under `threads` threads per workgroup; last < first: none"""
    slot_px = threads * 4
    n_slots = (c.cols * c.rows + slot_px - 1) // slot_px
    if c.res_range is None:
        return 0, n_slots - 1
    lo_inv, hi_p1 = c.res_range
    if hi_p1 == 0:
        return 0, -1
    sh = slot_px.bit_length() - 1 - 8
    return ((~lo_inv) & 0xffffffff) >> sh, min((hi_p1 - 1) >> sh, n_slots - 1)


def valid_set(c, threads):
    """what the compact residual pass finds under a launch shape -> valid bool [N] (candidate, pose-valid, inside a visited slot), the
    residual dictionary, count, and sum (int)(diff^2) as the wrapping 32-bit int of the reference"""
    r = residual(c)
    first, last = slot_range(c, threads)
    slot = np.arange(c.cols * c.rows) // (threads * 4)
    valid = r["ok"] & (np.asarray(c.cand, np.uint8).reshape(-1) != 0) & (slot >= first) & (slot <= last)
    count = int(valid.sum())
    sq = int((r["diff"][valid] ** 2).sum())      # (int)(diff * diff): diff is an integer of at most 255, its square exact in f32
    return valid, r, count, wrap32(sq), sq


def pack(k, g, diff):
    """the record of (k, g, diff) as the u64 the entry returns (x in the low word)"""
    return int(k) | ((int(g) | ((int(diff) + 256) << 22)) << 32)


def unpack(rec):
    rec = np.asarray(rec, np.uint64)
    xw = (rec & np.uint64(0xffffffff)).astype(np.int64); yw = (rec >> np.uint64(32)).astype(np.int64)
    return xw, yw & 0x3fffff, (yw >> 22) - 256


# ------------------------------------------------------------------------------------------------ sigma, F, rows
def sigma_val_from(count32, sigma32, rgb_only):
    """sigma handed to rgbStep (RGBDOdometry.cpp:373-385) from the two `int` totals: -1 in the RGB-only mode, 1 when tmpError ==
    sqrt(sigma) / count is 0 -- sigma == 0 and count != 0; 0 / 0 is NaN --, otherwise the COUNT (sic)"""
    if rgb_only:
        return F32(-1.0)
    return F32(1.0) if (sigma32 == 0 and count32 != 0) else F32(count32)


def rgb_fix_bits(sigma):
    """fraction bits of the sums: 8 for sigma == -1 or not >= 2, otherwise 8 + 2 * (biased exponent - 127) of sigma's f32 bits, at most 32"""
    sigma = F32(sigma)
    if sigma == F32(-1.0) or not (sigma >= F32(2.0)):
        return 8
    u = int(np.frombuffer(sigma.tobytes(), np.uint32)[0])
    return min(8 + 2 * (((u >> 23) & 255) - 127), 32)


def step_rows(c, valid, r, sigma):
    """rgb_step_row of every valid pixel, f32 in the kernel's operation order -> rows f32 [n, 7] in pixel order, and the intermediates"""
    k = np.flatnonzero(valid)
    g = r["g"][k]
    sigma = F32(sigma)
    diff = r["diff"][k].astype(F32)
    with np.errstate(all="ignore"):
        w = sigma + np.abs(diff)
        w = np.where(w > FLT_EPSILON, F32(1.0) / w, F32(1.0)).astype(F32)
        if sigma == F32(-1.0):
            w = np.ones_like(w)
        r6 = -w * diff
        cp = np.asarray(c.cloud, F32).reshape(-1, 3)[g]
        px, py, pz = cp[:, 0], cp[:, 1], cp[:, 2]
        invz = F32(1.0) / pz
        gx = w * F32(c.sobel) * np.asarray(c.dIdx, np.int16).reshape(-1)[k].astype(F32)
        gy = w * F32(c.sobel) * np.asarray(c.dIdy, np.int16).reshape(-1)[k].astype(F32)
        v0 = gx * F32(c.fx) * invz
        v1 = gy * F32(c.fy) * invz
        v2 = -(v0 * px + v1 * py) * invz
        rows = np.stack([v0, v1, v2, -pz * v1 + py * v2, pz * v0 - px * v2, -py * v0 + px * v1, r6], axis=1)
    assert rows.dtype == F32
    return rows, dict(w=w, invz=invz, gx=gx, gy=gy, pz=pz)


def exact_sums(rows, F):
    """the 29 sums in Python integers, NOT wrapped: 27 products i <= j over [row_0..5 | row_6], word 27 row_6^2, word 28 the count"""
    lim = Fraction(2) ** ((50 - F) // 2)
    scale = 1 << F
    sums = [0] * 29
    for row in rows:
        q = [min(max(Fraction(float(v)), -lim), lim) for v in row]
        k = 0
        for i in range(6):
            for j in range(i, 7):
                sums[k] += round(q[i] * q[j] * scale)    # round(Fraction): exact, half to even
                k += 1
        sums[27] += round(q[6] * q[6] * scale)
        sums[28] += 1
    return sums


def count_sum_ties(rows, F):
    """products of the (clamped) rows that are exact ties -- fraction exactly one half --, by sign"""
    lim = Fraction(2) ** ((50 - F) // 2)
    neg = pos = 0
    for row in rows:
        q = [min(max(Fraction(float(v)), -lim), lim) for v in row]
        for i in range(6):
            for j in range(i, 7):
                p = q[i] * q[j] * (1 << F)
                if p.denominator == 2:
                    neg += p < 0; pos += p > 0
    return int(neg), int(pos)


# ------------------------------------------------------------------------------------------------ one case under one launch shape
def reference(c, threads):
    """everything the GPU tests compare, for case `c` under `threads` threads per residual workgroup (the launch shape only matters to a
    ranged case: which slots are visited) -> dict"""
    valid, r, count, sq32, sq = valid_set(c, threads)
    assert sq < (1 << 31), "a slot's int sum of squares would wrap inside the kernel: outside what this reference states"
    add = 0 if c.no_counts else 1
    count_total = wrap64(sum(int(v) for v in c.count_seed) + add * count)
    sigma_total = wrap64(sum(int(v) for v in c.sigma_seed) + add * sq)
    sigma = sigma_val_from(wrap32(count_total), wrap32(sigma_total), c.rgb_only)
    F = rgb_fix_bits(sigma)
    rows, mid = step_rows(c, valid, r, sigma)
    sums = exact_sums(rows, F)
    first, last = slot_range(c, threads)
    slot_px = threads * 4
    n_slots = (c.cols * c.rows + slot_px - 1) // slot_px
    slots = {}
    for s in range(max(first, 0), last + 1):
        ks = np.flatnonzero(valid[s * slot_px:(s + 1) * slot_px]) + s * slot_px
        slots[s] = sorted(pack(k, r["g"][k], r["diff"][k]) for k in ks)
    return dict(valid=valid, res=r, count=count, sq32=sq32, count_total=count_total, sigma_total=sigma_total, sigma=sigma, F=F, rows=rows,
                mid=mid, sums=sums, sums64=np.array([wrap64(v) for v in sums] + [0, 0, 0], np.int64), first=first, last=last,
                n_slots=n_slots, slot_px=slot_px, slots=slots)
