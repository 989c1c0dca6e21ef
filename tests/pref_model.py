"""A NumPy model of the sweep pre-filter's builders, vector quantisers and interval formulas (no test in here).

It follows beta_cores_amd/csrc/bc_prefilter_i8.h, bc_prefilter_i4.h, bc_i8_quant.h and bc_i4_quant.h line by line -- float64 where
the device computes in fp64, float32 where it computes in fp32 (every NumPy operation on float32 arrays rounds once, as the
device code built with -ffp-contract=off does) -- and leaves its results in the DEVICE'S layouts (csrc/bc_layout.h), so that
the checker of tests/pref_cases.py reads a model run and a device run through the same code.  The model is not expected to be
bit-equal to the device (the approximate v_rcp / v_rsq of the 4-bit sweep are taken as correctly rounded, fma chains as plain
sums): the checker's tolerances cover that, and tests/test_pref_cases_cpu.py shows that they do not cover a wrong bound.

`doctor` names ONE deliberate defect (tests/test_pref_cases_cpu.py: DOCTORS); None is the faithful model.
"""
import numpy as np

F = np.float32
ITILE = 256
I4_DEAD, I4_UNCERTAIN = 255, 254
I4_SEEDS, I4_HOT = 256, 32


# ------------------------------------------------------------------ csrc/bc_layout.h restated
def lay_i8_sp4(S):
    return ((S + 3) // 4 + 4) // 5 * 5


def lay_i8_tiles(n):
    return max(1, (n + ITILE - 1) // ITILE)


def lay_i8_word(t, g, r, sp4):
    return t * sp4 * ITILE + g * ITILE + r


def lay_i4_groups(S):
    return (S + 7) // 8


def lay_i4_sp8(S, U):
    return (lay_i4_groups(S) + U - 1) // U * U


def lay_i4_batch(S):
    best = 13
    for c in (8, 7, 6, 5):
        if lay_i4_sp8(S, c) < lay_i4_sp8(S, best):
            best = c
    return best


def lay_i4_word(t, g, r, sp8):
    return t * sp8 * ITILE + g * ITILE + r


def lay_r8_bytes(S):
    return (4 * ((S + 3) // 4) + 4 + 127) // 128 * 128


def lay_phi_elem(row, k, S):
    return (row >> 7) * S * 128 + k * 128 + (row & 127)


# ------------------------------------------------------------------ small number-format helpers
def half_up(x):
    """The builders' "half rounded up": (_Float16)(float)x, stepped to the next half when that is below x (x > 0)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore'):
        h = x.astype(np.float32).astype(np.float16)
    low = h.astype(np.float64) < x
    bits = h.view(np.uint16) + low.astype(np.uint16)
    return bits.view(np.float16)


def ru32(x):
    """__double2float_ru"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        f = x.astype(np.float32)
        low = f.astype(np.float64) < x
        return np.where(low, np.nextafter(f, F(np.inf)), f).astype(np.float32)


def sext(x, bits):
    x = np.asarray(x).astype(np.int64) & ((1 << bits) - 1)
    return np.where(x >= (1 << (bits - 1)), x - (1 << bits), x).astype(np.int32)


# ------------------------------------------------------------------ builders
def build_i8(phi, norms, doctor=None):
    """k_build_i8 / k_build_i8_r: q [rows][4 sp4] int32 digits, (scale, delta) halfs.  phi: [n][S]; norms: [rows] (0 past n)."""
    n, S = phi.shape
    rows = norms.shape[0]
    sp4 = lay_i8_sp4(S)
    P = np.zeros((rows, S))
    P[:n] = phi
    live = (np.arange(rows) < n) & (norms != 0.)
    with np.errstate(all='ignore'):
        inr = np.where(live, 1. / np.where(live, norms, 1.), 0.)
        u = P * inr[:, None]
        has_nan = ~np.all(np.abs(u) <= 1.7976931348623157e308, axis=1)
        mx = np.where(has_nan, 0., np.max(np.where(np.isnan(u), 0., np.abs(u)), axis=1))
        ok = live & ~has_nan & (mx > 0.)
        t = np.where(ok, mx / 127., 1.)
        hs = half_up(t)
        if doctor == 'scale_nearest':
            hs = t.astype(np.float32).astype(np.float16)
        hs = np.where(hs.astype(np.float32) < F(6.2e-5), np.float16(F(6.2e-5)), hs)
        scale = np.where(ok, hs.astype(np.float64), 0.)
        iscale = np.where(ok, 1. / np.where(ok, scale, 1.), 0.)
        q = np.clip(np.rint(np.where(ok[:, None], u, 0.) * iscale[:, None]), -127, 127)
        d = np.where(ok[:, None], q * scale[:, None] - u, 0.)
        err2 = np.sum(d * d, axis=1)
        dd = np.sqrt(err2) * (1. + 1e-6) + 1e-12
        if doctor == 'delta_x095':
            dd = dd * 0.95
        hd = half_up(dd)
        if doctor == 'delta_nearest':
            hd = dd.astype(np.float32).astype(np.float16)
    qq = np.zeros((rows, 4 * sp4), dtype=np.int32)
    qq[:, :S] = np.where(ok[:, None], q, 0.).astype(np.int32)
    rowq = np.zeros((rows, 2), dtype=np.float16)
    rowq[:, 0] = np.where(ok, hs, np.float16(0.))
    rowq[:, 1] = np.where(ok, hd, np.float16(-1.))
    rowq[live & ~ok, 1] = np.uint16(0x7e00).view(np.float16)
    return qq, rowq


def build_i4(phi, norms, q8, rowq, doctor=None):
    """k_build_i4: nibbles [rows][8 sp8] and the 16-bit row codes.  The scale search runs on the int8 digits, as on the device."""
    n, S = phi.shape
    rows = norms.shape[0]
    U = lay_i4_batch(S)
    sp8 = lay_i4_sp8(S, U)
    g4 = (S + 3) // 4
    sc8 = rowq[:, 0].astype(np.float32)
    d8 = rowq[:, 1].astype(np.float32)
    dead, unc = d8 < 0, np.isnan(d8)
    with np.errstate(all='ignore'):
        cb = np.ceil(F(127.) * sc8 * F(1024. / 7.)).astype(np.float32)
        cb = np.clip(np.where(np.isfinite(cb), cb, 1), 1, 253).astype(np.int32)
        bestc = cb.copy()
        beste = np.full(rows, np.inf, dtype=np.float32)
        x8 = q8[:, :4 * g4].astype(np.float32)
        for f in range(8):
            c = (cb.astype(np.float32) * (F(1.) - F(0.1) * F(f)) + F(0.5)).astype(np.int32)
            c = np.maximum(c, 1)
            sc = c.astype(np.float32) * F(1. / 1024.)
            ratio = sc8 * (F(1024.) / c.astype(np.float32))
            x = x8 * ratio[:, None]
            qf = np.clip(np.rint(x), -7, 7).astype(np.float32)
            dq = qf - x
            e = np.sum((dq * dq).astype(np.float64), axis=1).astype(np.float32) * sc * sc
            better = e < beste
            beste = np.where(better, e, beste)
            bestc = np.where(better, c, bestc)
        scale = bestc.astype(np.float64) / 1024.
        iscale = 1024. / bestc.astype(np.float64)
        P = np.zeros((rows, 8 * sp8))
        P[:n, :S] = phi
        good = ~(dead | unc)
        inr = np.where(good, 1. / np.where(good, norms, 1.), 0.)
        u = np.where(good[:, None], P * inr[:, None], 0.)
        lim = 6 if doctor == 'i4_clip6' else 7
        q = np.clip(np.rint(u * iscale[:, None]), -lim, lim)
        d = q * scale[:, None] - u
        dd = np.sqrt(np.sum(d * d, axis=1)) * (1. + 1e-6) + 1e-12
        dc = np.ceil(dd * 512.)
    q = np.where(good[:, None], q, 0.).astype(np.int32)
    code = np.where(dc <= 250, bestc | (dc.astype(np.int64) << 8), I4_UNCERTAIN << 8)
    code = np.where(dead, I4_DEAD << 8, np.where(unc, I4_UNCERTAIN << 8, code))
    return q, code.astype(np.uint16)      # (a row whose measured error does not fit the code keeps its digits)


def pack_i8(q, ptiles, sp4):
    """[rows][4 sp4] digits -> the tile-major dwords [ptiles][sp4][256]"""
    b = (q.astype(np.int64) & 0xff).reshape(ptiles, ITILE, sp4, 4)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)
    return np.ascontiguousarray(w.transpose(0, 2, 1)).astype(np.uint32).view(np.int32).reshape(-1)


def pack_i4(q, ptiles, sp8):
    b = (q.astype(np.int64) & 0xf).reshape(ptiles, ITILE, sp8, 8)
    w = np.zeros(b.shape[:3], dtype=np.int64)
    for j in range(8):
        w |= b[..., j] << (4 * j)
    return np.ascontiguousarray(w.transpose(0, 2, 1)).astype(np.uint32).view(np.int32).reshape(-1)


def build_r8(q8, rowq, S, doctor=None):
    """k_build_r8: [rows][rb] bytes: ceil(S/4) dwords of digits, zeros, (scale, delta) in the last dword"""
    rows = q8.shape[0]
    rb, g4 = lay_r8_bytes(S), (S + 3) // 4
    r8 = np.zeros((rows, rb), dtype=np.uint8)
    off = 4 if doctor == 'r8_shifted' else 0
    r8[:, off:off + 4 * g4] = (q8[:, :4 * g4] & 0xff).astype(np.uint8)
    r8[:, rb - 4:] = rowq.view(np.uint8).reshape(rows, 4)
    return r8


# ------------------------------------------------------------------ vector quantisers
def _absmax(x):
    return np.inf if np.any(np.isnan(x)) else (float(np.max(np.abs(x))) if x.size else 0.)


def _split(v, S, mode):
    v = np.asarray(v, dtype=np.float64)
    return (v[0:2 * S:2], v[1:2 * S:2]) if mode == 0 else (v[:S], np.zeros(0))


def _header(S, vstep0, vstep1, vn, vbad, doctor):
    rs = float(np.sqrt(F(S))) * (0.5 * (1. + 1e-6))
    with np.errstate(all='ignore'):
        fev0, fev1 = ru32(rs * vstep0), ru32(rs * vstep1)
        if doctor == 'fev0_x09':
            fev0 = F(fev0 * F(0.9))
        if doctor == 'fev1_x09':
            fev1 = F(fev1 * F(0.9))
        return np.array([F(vstep0), F(vstep1), fev0, fev1, ru32(vn), F(1. if vbad else 0.), F(0.), F(0.)], dtype=np.float32)


def quant_i8(v, S, mode, doctor=None):
    """bc_i8q_wave: the record (4 sp4 ints of digits, 8 header floats)"""
    sp4 = lay_i8_sp4(S)
    v0, v1 = _split(v, S, mode)
    m0, m1 = _absmax(v0), (_absmax(v1) if mode == 0 else 0.)
    vbad = not (m0 < np.inf) or not (m1 < np.inf)
    with np.errstate(all='ignore'):
        vstep0, vstep1 = m0 * (1. / 16256.), m1 * (1. / 127.)
        r0 = 1. / m0 if (m0 > 0. and not vbad) else 0.
        r1 = 1. / m1 if (m1 > 0. and not vbad) else 0.
        inv0 = 16256. * r0 if vstep0 > 0. else 0.
        inv1 = 127. * r1 if vstep1 > 0. else 0.
    dig = np.zeros((4 * sp4, 3), dtype=np.int64)
    if not vbad:
        Q = np.clip(np.rint(v0 * inv0), -16256, 16256).astype(np.int64)
        d0 = np.rint(Q * 0.0078125).astype(np.int64)
        dig[:S, 0], dig[:S, 1] = d0, Q - 128 * d0
        if mode == 0:
            dig[:S, 2] = np.clip(np.rint(v1 * inv1), -127, 127).astype(np.int64)
    b = (dig & 0xff).reshape(sp4, 4, 3)
    w = np.zeros((sp4, 4), dtype=np.int64)
    for j in range(4):
        w[:, :3] |= b[:, j, :] << (8 * j)
    vn = 1. if mode == 0 else float(np.sqrt(np.sum(v0 * v0)))
    hdr = _header(S, vstep0, vstep1, vn, vbad, doctor)
    return np.concatenate((w.astype(np.uint32).view(np.int32).reshape(-1), hdr.view(np.int32)))


def quant_i4(v, S, mode, doctor=None):
    """bc_i4q_wave"""
    sp8 = lay_i4_sp8(S, lay_i4_batch(S))
    v0, v1 = _split(v, S, mode)
    m0, m1 = _absmax(v0), (_absmax(v1) if mode == 0 else 0.)
    vbad = not (m0 < np.inf) or not (m1 < np.inf)
    with np.errstate(all='ignore'):
        vstep = [m0 * (1. / 119.), m1 * (1. / 119.)]
        inv = [119. * (1. / m) if (m > 0. and not vbad and m * (1. / 119.) > 0.) else 0. for m in (m0, m1)]
    dig = np.zeros((8 * sp8, 4), dtype=np.int64)
    if not vbad:
        for vv, x in enumerate((v0, v1) if mode == 0 else (v0,)):
            Q = np.clip(np.rint(x * inv[vv]), -119, 119).astype(np.int64)
            d0 = (Q + 8) >> 4
            dig[:S, 2 * vv], dig[:S, 2 * vv + 1] = d0, Q - 16 * d0
    b = (dig & 0xf).reshape(sp8, 8, 4)
    w = np.zeros((sp8, 4), dtype=np.int64)
    for j in range(8):
        w |= b[:, j, :] << (4 * j)
    vn = 1. if mode == 0 else float(np.sqrt(np.sum(v0 * v0)))
    hdr = _header(S, vstep[0], vstep[1], vn, vbad, None)
    return np.concatenate((w.astype(np.uint32).view(np.int32).reshape(-1), hdr.view(np.int32)))


def record_digits(rec, groups, per):
    """The digits of a record's `groups` k-groups of `per` samples: [groups * per][4] (one column per packed word)."""
    w = rec[:4 * groups].view(np.uint32).astype(np.int64).reshape(groups, 4)
    bits = 32 // per
    out = np.zeros((groups, per, 4), dtype=np.int32)
    for j in range(per):
        out[:, j, :] = sext(w >> (bits * j), bits)
    return out.reshape(groups * per, 4)


def record_header(rec, groups):
    return rec[4 * groups:4 * groups + 8].view(np.float32)


# ------------------------------------------------------------------ the interval formulas in fp32
def interval_f32(mode, s0, s1, delta0, delta1, pd, hw, doctor=None):
    """bc_score_interval_f32 (hw: bc_score_interval_f32_hw, its approximate reciprocals taken as correctly rounded)"""
    s0, s1, delta0, delta1 = (np.asarray(x, dtype=np.float32) for x in (s0, s1, delta0, delta1))
    fe = F(1e-6) if hw else F(6e-7)
    with np.errstate(all='ignore'):
        if mode == 0:
            a = np.abs(s1) + delta1
            c = F(1.) - a * a
            bad = np.isnan(s0) | np.isnan(s1) | ~(c > F(1e-3))
            cc = np.where(bad, F(1.), c)
            rc2 = (F(1.) / cc) * F(1.000001)
            rc = np.sqrt(rc2) * F(1.000001)
            g = np.where(bad, F(1.), F(1.) - s1 * s1)
            f = s0 * (1. / np.sqrt(g.astype(np.float64))).astype(np.float32)
            slope = (np.abs(s0) + delta0) * a * delta1 * rc * rc2
            if doctor == 'no_slope':
                slope = slope * F(0.)
            e = (delta0 * rc + slope) * F(1.003) + np.abs(f) * (F(6.1e-8) * rc2 + fe) + F(2e-7)
        else:
            bad = np.isnan(s0)
            pd = F(pd)
            ip = (F(1.) / np.abs(pd)) * F(1.000001)
            f = s0 / pd
            e = (delta0 * F(1.002) + F(3e-7) * np.abs(s0)) * ip + (F(1e-6) if hw else F(2e-7)) * np.abs(f) + F(1e-30)
        U = np.where(bad, F(np.inf), f + e).astype(np.float32)
        L = np.where(bad, F(-np.inf), f - e).astype(np.float32)
    return U, L


def sweep_i8(mode, q8, rowq, rec8, S, pd, doctor=None, shift=0):
    """k_sweep_i8's per-row evaluation (bc_i8_row_bounds) for every row: (U, L) float32 [rows][2].  shift: the doctored level 2
    reads the (scale, delta) of row i + shift."""
    sp4 = lay_i8_sp4(S)
    dg = record_digits(rec8, sp4, 4).astype(np.int64)
    h = record_header(rec8, sp4)
    A = q8.astype(np.int64).dot(dg[:, :3])
    rq = np.roll(rowq, -shift, axis=0) if shift else rowq
    sc, dr = rq[:, 0].astype(np.float32), rq[:, 1].astype(np.float32)
    fvs0, fvs1, fev0, fev1, fvn, vbad = h[0], h[1], h[2], h[3], h[4], h[5] != 0
    with np.errstate(all='ignore'):
        s0 = sc * fvs0 * (F(128.) * A[:, 0].astype(np.float32) + A[:, 1].astype(np.float32))
        s1 = sc * fvs1 * A[:, 2].astype(np.float32) if mode == 0 else np.zeros_like(s0)
        d0 = (dr * fvn + (F(1.) + dr) * fev0) * F(1.00001) + F(4e-7) * np.abs(s0) + F(1e-12)
        d1 = (dr * fvn + (F(1.) + dr) * fev1) * F(1.00001) + F(4e-7) * np.abs(s1) + F(1e-12) if mode == 0 else np.zeros_like(s0)
        U, L = interval_f32(mode, s0, s1, d0, d1, pd, False, doctor)
    unc = vbad | np.isnan(dr)
    U = np.where(unc, F(np.inf), U)
    L = np.where(unc, F(-np.inf), L)
    dead = dr < 0
    U = np.where(dead, F(-np.inf), U)
    L = np.where(dead, F(-np.inf), L)
    return np.stack((U, L), axis=1).astype(np.float32)


def sweep_i4(mode, q4, code, rec4, S, pd, doctor=None):
    """k_sweep_i4's epilogue for every row"""
    sp8 = lay_i4_sp8(S, lay_i4_batch(S))
    dg = record_digits(rec4, sp8, 8).astype(np.int64)
    h = record_header(rec4, sp8)
    A = q4.astype(np.int64).dot(dg)
    dc = (code >> 8).astype(np.int32)
    sc = (code & 0xff).astype(np.float32) * F(1. / 1024.)
    dr = dc.astype(np.float32) * F(1. / 512.)
    fvs0, fvs1, fev0, fev1, fvn, vbad = h[0], h[1], h[2], h[3], h[4], h[5] != 0
    with np.errstate(all='ignore'):
        s0 = sc * fvs0 * (F(16.) * A[:, 0].astype(np.float32) + A[:, 1].astype(np.float32))
        s1 = sc * fvs1 * (F(16.) * A[:, 2].astype(np.float32) + A[:, 3].astype(np.float32)) if mode == 0 else np.zeros_like(s0)
        d0 = (dr * fvn + (F(1.) + dr) * fev0) * F(1.00001) + F(4e-7) * np.abs(s0) + F(1e-12)
        d1 = (dr * fvn + (F(1.) + dr) * fev1) * F(1.00001) + F(4e-7) * np.abs(s1) + F(1e-12) if mode == 0 else np.zeros_like(s0)
        U, L = interval_f32(mode, s0, s1, d0, d1, pd, True, doctor)
    dead, unc = dc == I4_DEAD, vbad | (dc == I4_UNCERTAIN)
    U = np.where(dead, F(-np.inf), np.where(unc, F(np.inf), U))
    L = np.where(dead | unc, F(-np.inf), L)
    return np.stack((U, L), axis=1).astype(np.float32)


# ------------------------------------------------------------------ a whole run, in the device's layouts
class Snap(dict):
    """What a run leaves behind, by the names of bc_snnls_prefdiag_copy, in the device's layouts."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def device_norms(phi, rows):
    nr = np.zeros(rows)
    with np.errstate(all='ignore'):
        nr[:phi.shape[0]] = np.sqrt(np.sum(phi * phi, axis=1))
    return nr


def run_model(phi, mode, v, pd=1.0, seeds=None, v_prev=None, doctor=None, two_level=True, mirrors=None):
    """Both mirrors, both digit records and every row's intervals for one sweep vector.  seeds: rows whose level-2 lower bounds
    make theta0 (None: no two-level outputs).  v_prev: the vectors of the step before (only the doctored theta0 reads them)."""
    n, S = phi.shape
    ptiles = lay_i8_tiles(n)
    rows = ptiles * ITILE
    norms = device_norms(phi, rows)
    two_level = two_level and S <= 256
    s = Snap(S=S, n=n, mode=mode, post_div=float(pd), phi=phi, norms=norms, ptiles=ptiles, sp4=lay_i8_sp4(S), two=two_level,
             v=np.asarray(v, dtype=np.float64).copy())
    mirrors = {} if mirrors is None else mirrors            # (a cache the caller keeps per matrix and doctor)
    if 'i8' not in mirrors:
        mirrors['i8'] = build_i8(phi, norms, doctor)
    q8, rowq = mirrors['i8']
    if 'u8' not in mirrors:
        mirrors['u8'] = pack_i8(q8, ptiles, s.sp4)
    s.u8, s.rowq = mirrors['u8'], rowq.view(np.uint16).reshape(-1).copy()
    s.qv = quant_i8(v, S, mode, doctor)
    s.ul_i8 = sweep_i8(mode, q8, rowq, s.qv, S, pd, doctor)
    if two_level:
        s.i4_u = lay_i4_batch(S)
        s.sp8, s.g4, s.rb = lay_i4_sp8(S, s.i4_u), (S + 3) // 4, lay_r8_bytes(S)
        if 'i4' not in mirrors:
            mirrors['i4'] = build_i4(phi, norms, q8, rowq, doctor)
        q4, code = mirrors['i4']
        if 'u4' not in mirrors:
            mirrors['u4'], mirrors['r8'] = pack_i4(q4, ptiles, s.sp8), build_r8(q8, rowq, S, doctor).reshape(-1)
        s.u4, s.rowq4, s.r8 = mirrors['u4'], code, mirrors['r8']
        s.qv4 = quant_i4(v, S, mode, doctor)
        s.ul_i4 = sweep_i4(mode, q4, code, s.qv4, S, pd, doctor)
        if seeds is not None:
            l2 = sweep_i8(mode, q8, rowq, s.qv, S, pd, doctor, shift=1 if doctor == 'l2_next_row' else 0)
            seed_src = l2
            if doctor == 'theta0_stale':
                seed_src = sweep_i8(mode, q8, rowq, quant_i8(v_prev, S, mode), S, pd)
            ls = seed_src[np.asarray(seeds, dtype=np.int64), 1]
            ls = ls[~np.isnan(ls)]
            theta0 = F(max([F(-np.inf)] + list(ls)))
            passed = (s.ul_i4[:, 0] >= theta0) & (s.ul_i4[:, 0] != F(-np.inf))
            s.ul8 = np.where(passed[:, None], l2, F(np.nan)).astype(np.float32)
            s.theta0 = np.full(4, theta0, dtype=np.float32)
    return s
