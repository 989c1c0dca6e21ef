"""The sweep pre-filter's chain of inequalities, link by link: reference, checker and cases (no test in here).

DESIGN.md section 4 says the selections of the int8 sweep (k_sweep_i8) and of the two-level form (k_sweep_i4) equal the fp64
sweep's "by construction".  The construction is a chain -- the mirrors' per-row delta is at least the measured quantisation
error; the vector records' fev0 / fev1 / fvn are at least the true norms; [L_i, U_i] contains the score bc_row_score computes;
theta0 is a lower bound of the best exact score; level 2 produces the int8 sweep's bounds -- and this module checks every link
from what a run leaves behind (`Snap`, tests/pref_model.py: the buffers of bc_snnls_prefdiag_copy and the per-row output of
bc_snnls_prefdiag_sweep, in the device's layouts), whether the run was the NumPy model's (tests/test_pref_cases_cpu.py) or the
device's (tests/test_gpu_pref_bounds.py).  Everything is evaluated in np.longdouble from the host Phi, the device's norms and
the vectors actually swept.

Reference.  f_i = bc_row_score (csrc/bc_sweep_dev.h) restated with u = Phi_i / norm_i, the validity mask and post_div.  The fp64
kernel's own fma chain may move its dot products by at most (S + 3) 2^-53 sum_k |Phi_ik v_k| / norm_i; that is pushed through
the epilogue (mean value theorem, as the bound itself) and ALLOWED on either side of [L, U].  `check_intervals` asserts that
the allowance stays below 1e-3 of the smallest finite half-width it meets, so it cannot hide a violation.

Tightness.  For a finite interval the half-width must equal the documented formula (bc_score_interval_f32 / _hw with their
inflation constants, delta0 / delta1 of bc_i8_row_bounds) evaluated in longdouble from the row's STORED delta and the record's
header: relative 1e-4 plus 1e-6 (1 + |f|) for the fp32 evaluation.  So a bound that is sound only because it is vacuous fails.

Adversarial vectors.  On random vectors the Cauchy-Schwarz bounds are 2-5x slack: a delta understated threefold passes.  The
cases below make one term of the bound nearly attained (attainment = |centre - f| / half-width of the targeted row):
  row    dot mode, v along e_i = q_i scale_i - u_i of chosen rows i (the 4-bit form: e4_i): the term delta_i ||v||;
  vec    dot mode, a row that the int8 mirror represents to 1e-6 (integer entries q_k with sum q_k^2 just above 1 / h^2 for a
         half h: u_k = q_k / ||q||, scale = h, delta ~ 1e-6; nearly equal |q_k| so that Cauchy-Schwarz is tight) against a v
         whose entries sit just below half-steps, (Q_k + 0.4999 |q_k| / 127) vstep, signed like the row: the term sqrt(S) vstep / 2;
  slope  GIGA, the same row: v0 = u (|s0| = 1) and v1 at half-steps of its single digit with s1 ~ 0.5: the term
         (|s0| + delta0) a delta1 / c^(3/2).
  (An all-+-1/sqrt(S) row does NOT work for `vec` / `slope`: its scale is the first half above 1 / (127 sqrt(S)), up to 1e-3
  off, and the row term delta_i ||v|| >= delta_i 16256 vstep then swamps sqrt(S) vstep / 2.  Hence the integer construction.)
Further rows of every case matrix (n >= 64): a ladder of rows at angles to v1 whose c = 1 - (|s1| + delta1)^2 lies on both sides
of the 1e-3 threshold (both levels), a row parallel to v1 (s1 = 1: masked by the reference), a zero row, a NaN row, an inf
row; and one vector holding a NaN.

Attainment of the targeted term (best targeted row of a case matrix; then the WORST case matrix of the list): the NumPy model
(tests/test_pref_cases_cpu.py asserts >= 0.9 for S >= 37 and >= 0.8 for S = 8 on row, vec and slope, >= 0.8 on row4) and one
MI355X (tests/test_gpu_pref_bounds.py prints them; they agree with the model to four digits, S = 8 includes its 1-row matrix):

  term                          model S >= 37   model S = 8   device S >= 37      device S = 8
  row    delta_i ||v||, int8    0.9871          0.9776        0.9871 .. 0.9920    0.9711
  row4   the same, 4-bit        0.8007          0.8707        0.8007 .. 0.9302    0.8550
  vec    sqrt(S) vstep / 2      0.9352          0.8347        0.9352 .. 0.9717    0.8347
  slope  (|s0|+d0) a d1/c^1.5   0.9182          0.8217        0.9182 .. 0.9532    0.8217
  (row4 stops near 0.9: delta4 is coded in steps of 1 / 512 and the 4-bit vector record's own sqrt(S) vstep / 2 is 5-10 % of
  delta4 ||v||.  vec and slope lose (RMS q / 127) (S - 1) / S to the row's unequal entries and to the exact maximum element.)

Worst |centre - f| / half-width over every row of every case and of the solver's own vectors, device: int8 sweep 0.992, level 2
0.992, 4-bit level 0.930 -- no interval was violated, and none is vacuous: the half-width equals the documented formula within
the tolerance above on every finite row.  On random vectors the worst row reaches 0.3-0.5 (S >= 37).

Tightness, one correction to the reference (the code is deliberate): c = 1 - a * a is formed in fp32 with an absolute error
<= 3 * 2^-24, which the c^(-3/2) of the slope term turns into a relative 4.5 * 2^-24 / c of the half-width -- 1.3e-4 at
c = 2e-3.  The tolerance carries that derived term beside the 1e-4 and the 1e-6 (1 + |f|); without it a sound, documented
bound fails on the ladder rows just above the 1e-3 threshold (seen on the model, whose fp32 arithmetic is the device's).  Likewise fvn >= ||v|| is asked up to the
(S + 2) 2^-53 of the fp64 norm it is rounded up from.
"""
import functools
from fractions import Fraction
from math import isqrt

import numpy as np

import pref_model as M
from two_level_shapes import S_LIST

LD = np.longdouble
EXTRA_S = [1, 5, 8, 104, 105, 300]
N_LIST = [1, 255, 256, 257, 300, 3001]


def fail(what, fmt, *args):
    raise AssertionError('%s: %s' % (what, fmt % args))


# ------------------------------------------------------------------ decoding the device's layouts (formulas of csrc/bc_layout.h)
def decode_i8(s):
    t, g, r = np.meshgrid(np.arange(s.ptiles), np.arange(s.sp4), np.arange(M.ITILE), indexing='ij')
    w = s.u8.view(np.uint32)[M.lay_i8_word(t, g, r, s.sp4)].astype(np.int64)          # [ptiles][sp4][256]
    q = np.stack([M.sext(w >> (8 * j), 8) for j in range(4)], axis=-1)              # [..][4]
    return q.transpose(0, 2, 1, 3).reshape(s.ptiles * M.ITILE, 4 * s.sp4)


def decode_i4(s):
    t, g, r = np.meshgrid(np.arange(s.ptiles), np.arange(s.sp8), np.arange(M.ITILE), indexing='ij')
    w = s.u4.view(np.uint32)[M.lay_i4_word(t, g, r, s.sp8)].astype(np.int64)
    q = np.stack([M.sext(w >> (4 * j), 4) for j in range(8)], axis=-1)
    return q.transpose(0, 2, 1, 3).reshape(s.ptiles * M.ITILE, 8 * s.sp8)


def rows_of(s):
    return s.ptiles * M.ITILE


def unit_rows(s):
    """u = Phi / norm in longdouble [rows][S] (0 for dead rows), and the row classes: live, holding a NaN / inf."""
    rows = rows_of(s)
    live = (np.arange(rows) < s.n) & (s.norms != 0.)
    u = np.zeros((rows, s.S), dtype=LD)
    with np.errstate(all='ignore'):
        u[:s.n] = s.phi.astype(LD) / np.where(live[:s.n], s.norms[:s.n], 1.).astype(LD)[:, None]
    u[~live] = 0
    bad = live & ~np.all(np.isfinite(u.astype(np.float64)), axis=1)
    return u, live, bad


# ------------------------------------------------------------------ the mirrors
def check_mirror_i8(s):
    what = 'int8 mirror'
    u, live, bad = unit_rows(s)
    q = decode_i8(s)
    rq = s.rowq.view(np.float16).reshape(-1, 2)
    bits = s.rowq.reshape(-1, 2)
    scale, delta = rq[:, 0].astype(LD), rq[:, 1].astype(LD)
    S = s.S
    if np.any(q[:, S:] != 0):
        fail(what, 'padding digits or k-groups up to sp4 are not zero (row %d)', np.argmax(np.any(q[:, S:] != 0, axis=1)))
    dead = ~live
    if np.any(rq[dead, 1] != np.float16(-1.)) or np.any(q[dead] != 0) or np.any(rq[dead, 0] != 0):
        fail(what, 'a dead row does not carry delta = -1 and zero digits')
    if not np.all(np.isnan(rq[bad, 1])) or np.any(q[bad] != 0):
        fail(what, 'a row holding NaN / inf does not carry a NaN delta and zero digits')
    ok = live & ~bad
    if np.any(np.abs(q) > 127):
        fail(what, '|q| > 127')
    ex = (bits[:, 0] >> 10) & 0x1f
    if np.any(ok & ((ex == 0) | (ex == 31) | (bits[:, 0] >> 15 != 0))):
        fail('int8 scale', 'not a normal positive half (row %d)', np.argmax(ok & ((ex == 0) | (ex == 31))))
    mx = np.max(np.abs(u), axis=1)
    t = mx / LD(127)
    floor_h = np.float16(np.float32(6.2e-5))
    at_floor = rq[:, 0] == floor_h
    prev = (bits[:, 0] - 1).astype(np.uint16).view(np.float16).astype(LD)
    small = ok & ~at_floor & (scale * (1 + LD(4e-16)) < t)
    if np.any(small):
        i = int(np.argmax(small))
        fail('int8 scale', 'row %d: %.9g is below max|u| / 127 = %.9g (not the first half at or above it)', i, float(scale[i]), float(t[i]))
    large = ok & ~at_floor & (prev >= t * (1 + LD(4e-16)))
    if np.any(large):
        i = int(np.argmax(large))
        fail('int8 scale', 'row %d: %.9g is more than one half above max|u| / 127 = %.9g', i, float(scale[i]), float(t[i]))
    if np.any(ok & at_floor & (t > scale)):
        fail('int8 scale', 'a row at the floor 6.2e-5 whose max|u| / 127 is above it')
    e = np.where(ok[:, None], q[:, :S].astype(LD) * scale[:, None] - u, 0)
    over = ok[:, None] & (np.abs(e) > scale[:, None] / 2 * (1 + LD(1e-12)))
    if np.any(over):
        i = int(np.argmax(np.any(over, axis=1)))
        fail('int8 digit', 'row %d: |q scale - u| = %.6g > scale / 2 = %.6g', i, float(np.max(np.abs(e[i]))), float(scale[i] / 2))
    en = np.sqrt(np.sum(e * e, axis=1))
    low = ok & (delta < en)
    if np.any(low):
        i = int(np.argmax(np.where(low, en / np.maximum(delta, LD(1e-300)), 0)))
        fail('int8 delta below the measured error', 'row %d: delta %.9g < ||q scale - u|| = %.9g (%d rows)', i, float(delta[i]), float(en[i]),
             int(low.sum()))
    X = (en * (1 + LD(1e-6)) + LD(1e-12)).astype(np.float64)
    hx = M.half_up(X * (1 - 1e-12))
    cap = (hx.view(np.uint16) + 1).astype(np.uint16).view(np.float16).astype(LD)
    high = ok & (delta > cap)
    if np.any(high):
        i = int(np.argmax(high))
        fail('int8 delta too wide', 'row %d: delta %.9g is more than a half-step above %.9g', i, float(delta[i]), float(X[i]))
    return dict(u=u, live=live, bad=bad, q=q, scale=scale, delta=delta, e=e, en=en)


def check_mirror_i4(s):
    what = '4-bit mirror'
    u, live, bad = unit_rows(s)
    q = decode_i4(s)
    S = s.S
    code = s.rowq4.astype(np.int64)
    c, dc = code & 0xff, code >> 8
    if np.any(q == -8):
        fail('4-bit digit', 'a nibble of -8')
    if np.any(q[:, S:] != 0):
        fail(what, 'padding nibbles or k-groups up to sp8 are not zero')
    if np.any(dc[~live] != M.I4_DEAD) or np.any(q[~live] != 0):
        fail(what, 'a dead row does not carry code 255 and zero digits')
    if np.any(dc[bad] != M.I4_UNCERTAIN) or np.any(q[bad] != 0):
        fail(what, 'a row holding NaN / inf does not carry code 254 and zero digits')
    ok = live & ~bad
    scale = c.astype(LD) / 1024
    e = np.where(ok[:, None], q[:, :S].astype(LD) * scale[:, None] - u, 0)
    en = np.sqrt(np.sum(e * e, axis=1))
    coded = ok & (dc <= 250)
    if np.any(ok & ~coded & ((dc != M.I4_UNCERTAIN) | (en * 512 <= 249))):
        fail(what, 'a finite row is marked uncertain although its measured error fits the delta code')
    if np.any(coded & ((c < 1) | (c > 253))):
        fail('4-bit scale', 'scale code outside 1 .. 253')
    a = np.abs(u) / np.where(coded, scale, 1)[:, None]
    qa = np.abs(q[:, :S])
    inner = coded[:, None] & (qa < 7) & (np.abs(e) > scale[:, None] / 2 * (1 + LD(1e-12)))
    edge = coded[:, None] & (qa == 7) & ((a < LD(6.5) * (1 - LD(1e-12))) | (np.sign(q[:, :S]) != np.sign(u)))
    if np.any(inner | edge):
        i, k = np.argwhere(inner | edge)[0]
        fail('4-bit digit', 'row %d sample %d: digit %d for u / scale = %.6f is not clamp(rint(.), +-7)', i, k, q[i, k], float(u[i, k] / scale[i]))
    d4 = dc.astype(LD) / 512
    low = coded & (d4 < en)
    if np.any(low):
        i = int(np.argmax(low))
        fail('4-bit delta below the measured error', 'row %d: delta4 %.9g < ||q scale - u|| = %.9g', i, float(d4[i]), float(en[i]))
    high = coded & (d4 > en * (1 + LD(1e-6)) + LD(1e-12) + LD(1) / 512)
    if np.any(high):
        i = int(np.argmax(high))
        fail('4-bit delta too wide', 'row %d: delta4 %.9g against a measured error of %.9g', i, float(d4[i]), float(en[i]))
    return dict(u=u, live=live, bad=bad, q=q, scale=scale, delta=d4, code=dc, e=e, en=en)


def check_r8(s):
    q = decode_i8(s)
    g4 = (s.S + 3) // 4
    r8 = s.r8.reshape(-1, s.rb)
    if s.rb != M.lay_r8_bytes(s.S) or r8.shape[0] != rows_of(s):
        fail('r8 record', 'rb = %d for S = %d', s.rb, s.S)
    if not np.array_equal(r8[:, :4 * g4].view(np.int8).astype(np.int32), q[:, :4 * g4]):
        i = int(np.argmax(np.any(r8[:, :4 * g4].view(np.int8) != q[:, :4 * g4], axis=1)))
        fail('r8 record', "row %d: its bytes are not the row's int8 digits", i)
    if not np.array_equal(r8[:, s.rb - 4:].reshape(-1), s.rowq.view(np.uint8)):
        fail('r8 record', "the last dword is not the row's (scale, delta)")
    if np.any(r8[:, 4 * g4:s.rb - 4] != 0):
        fail('r8 record', 'the bytes between the digits and the last dword are not zero')


# ------------------------------------------------------------------ the vector records
def split_v(s):
    v = np.asarray(s.v, dtype=np.float64)
    return (v[0:2 * s.S:2], v[1:2 * s.S:2]) if s.mode == 0 else (v[:s.S], None)


def check_record(s, level):
    """What tests/i4_quant_harness.cpp checks on the host, on the record actually swept; in addition fvn >= ||v||."""
    what = 'int8 record' if level == 'i8' else '4-bit record'
    S, mode = s.S, s.mode
    groups, per = (s.sp4, 4) if level == 'i8' else (s.sp8, 8)
    rec = s.qv if level == 'i8' else s.qv4
    dg = M.record_digits(rec, groups, per).astype(np.int64)
    h = M.record_header(rec, groups).astype(LD)
    v0, v1 = split_v(s)
    vbad = not np.all(np.isfinite(v0)) or (v1 is not None and not np.all(np.isfinite(v1)))
    if (h[5] != 0) != vbad:
        fail(what, 'vbad = %g for a vector that %s NaN / inf', float(h[5]), 'holds' if vbad else 'holds no')
    if vbad:
        if np.any(dg != 0):
            fail(what, 'a bad vector must carry no digits')
        return None
    if np.any(dg[S:] != 0):
        fail(what, 'padding digits are not zero')
    out = {}
    for vv, x in enumerate((v0, v1) if mode == 0 else (v0,)):
        step = h[vv]
        if level == 'i8' and vv == 0:
            d0, d1 = dg[:S, 0], dg[:S, 1]
            if np.any(np.abs(d0) > 127) or np.any(np.abs(d1) > 64):
                fail(what, 'digits out of range')
            Q, qmax = 128 * d0 + d1, 16256
        elif level == 'i8':
            Q, qmax = dg[:S, 2], 127
        else:
            d0, d1 = dg[:S, 2 * vv], dg[:S, 2 * vv + 1]
            if np.any(np.abs(d0) > 7) or np.any(d1 < -8) or np.any(d1 > 7):
                fail(what, 'nibbles out of range')
            Q, qmax = 16 * d0 + d1, 119
        if np.any(np.abs(Q) > qmax):
            fail(what, '|Q| > %d', qmax)
        mx = LD(np.max(np.abs(x))) if S else LD(0)
        true_step = mx / qmax
        if abs(step - true_step) > LD(1.3e-7) * true_step + LD(1e-300):
            fail(what, 'step %d: %.9g against max|v| / %d = %.9g', vv, float(step), qmax, float(true_step))
        err = Q.astype(LD) * true_step - x.astype(LD)
        if np.any(np.abs(err) > true_step / 2 * (1 + LD(1e-11)) + LD(1e-300)):
            fail(what, 'a digit of vector %d is off by more than half a step', vv)
        en = np.sqrt(np.sum(err * err))
        if h[2 + vv] < en:
            fail('fev%d' % vv, '%s: fev%d = %.9g < ||v^ - v|| = %.9g', what, vv, float(h[2 + vv]), float(en))
        out['err%d' % vv] = en
    if mode == 1 and np.any(dg[:, 2:] != 0):
        fail(what, 'dot mode: the second vector must stay empty')
    vn = np.sqrt(np.sum(v0.astype(LD) ** 2)) if mode == 1 else max(np.sqrt(np.sum(v0.astype(LD) ** 2)), np.sqrt(np.sum(v1.astype(LD) ** 2)))
    # fvn is the fp64 norm rounded UP to fp32: the fp64 sum of S squares and its root carry (S + 2) 2^-53 (the 1.00001 the
    # sweeps inflate delta by is nine orders above that); GIGA's vectors are unit vectors to 1e-9 and fvn = 1
    if h[4] < vn * (1 - (LD(2e-9) if mode == 0 else LD(S + 2) * LD(2) ** -53)):
        fail('fvn', '%s: fvn = %.17g < ||v|| = %.17g', what, float(h[4]), float(vn))
    return out


# ------------------------------------------------------------------ the exact scores
def exact_scores(s, u):
    """f (longdouble), the allowance for the fp64 kernel's own rounding, and s1 with its allowance (GIGA)."""
    v0, v1 = split_v(s)
    S = s.S
    eps = LD(S + 3) * LD(2) ** -53
    with np.errstate(all='ignore'):
        s0 = u.dot(v0.astype(LD))
        a0 = eps * np.abs(u).dot(np.abs(v0).astype(LD))
        if s.mode == 1:
            return s0 / LD(s.post_div), a0 / abs(LD(s.post_div)) + LD(4) * LD(2) ** -53 * np.abs(s0 / LD(s.post_div)), None
        s1 = u.dot(v1.astype(LD))
        a1 = eps * np.abs(u).dot(np.abs(v1).astype(LD))
        ok = (s1 > -1 + LD(1e-14)) & (1 - s1 * s1 > 0)
        den = np.where(ok, np.sqrt(np.where(ok, 1 - s1 * s1, 1)), LD(np.inf))
        f = s0 / den
        c = 1 - (np.abs(s1) + a1) ** 2
        cc = np.where(c > 0, c, 1)
        allow = np.where(ok, a0 / np.sqrt(cc) + np.abs(s0) * (np.abs(s1) + a1) * a1 / cc ** LD(1.5) + LD(6) * LD(2) ** -53 * np.abs(f), 0)
        allow = np.where(ok & ~(c > 0), LD(np.inf), allow)
    return f, allow, s1


def documented(s, level, mir, hw):
    """The documented interval in longdouble from the STORED digits, scales, deltas and the record's header."""
    groups, per = (s.sp4, 4) if level == 'i8' else (s.sp8, 8)
    rec = s.qv if level == 'i8' else s.qv4
    dg = M.record_digits(rec, groups, per).astype(np.int64)
    h = M.record_header(rec, groups).astype(LD)
    A = mir['q'].astype(np.int64).dot(dg)
    sc, dr = mir['scale'], mir['delta']
    with np.errstate(all='ignore'):
        if level == 'i8':
            s0 = sc * h[0] * (128 * A[:, 0] + A[:, 1]).astype(LD)
            s1 = sc * h[1] * A[:, 2].astype(LD)
        else:
            s0 = sc * h[0] * (16 * A[:, 0] + A[:, 1]).astype(LD)
            s1 = sc * h[1] * (16 * A[:, 2] + A[:, 3]).astype(LD)
        d0 = (dr * h[4] + (1 + dr) * h[2]) * LD(1.00001) + LD(4e-7) * np.abs(s0) + LD(1e-12)
        d1 = (dr * h[4] + (1 + dr) * h[3]) * LD(1.00001) + LD(4e-7) * np.abs(s1) + LD(1e-12)
        if s.mode == 0:
            a = np.abs(s1) + d1
            c = 1 - a * a
            cc = np.where(c > 0, c, 1)
            rc2 = 1 / cc * LD(1.000001)
            rc = np.sqrt(rc2) * LD(1.000001)
            g = 1 - s1 * s1
            f = s0 / np.sqrt(np.where(g > 0, g, 1))
            term_row = dr * h[4] * rc
            term_vec = (1 + dr) * h[2] * rc
            term_slope = (np.abs(s0) + d0) * a * d1 * rc * rc2
            e = (d0 * rc + term_slope) * LD(1.003) + np.abs(f) * (LD(6.1e-8) * rc2 + LD(1e-6 if hw else 6e-7)) + LD(2e-7)
        else:
            pd = LD(s.post_div)
            ip = 1 / abs(pd) * LD(1.000001)
            f = s0 / pd
            c = np.ones_like(s0)
            term_row, term_vec, term_slope = dr * h[4] * ip, (1 + dr) * h[2] * ip, np.zeros_like(s0)
            e = (d0 * LD(1.002) + LD(3e-7) * np.abs(s0)) * ip + LD(1e-6 if hw else 2e-7) * np.abs(f) + LD(1e-30)
    return dict(f=f, e=e, c=c, vbad=h[5] != 0, terms=dict(row=term_row, vec=term_vec, slope=term_slope))


def check_intervals(s, ul, level, mir, hw, what, only=None):
    """Containment, tightness, dead rows and uncertain rows of every row of `ul` ([rows][2] float32 (U, L)); only: a row mask
    (level 2: the rows it re-bounded).  Returns the figures a test prints."""
    u, live, bad = mir['u'], mir['live'], mir['bad']
    f, allow, _ = s['_exact'] if '_exact' in s else exact_scores(s, u)
    doc = documented(s, level, mir, hw)
    U, L = ul[:, 0].astype(LD), ul[:, 1].astype(LD)
    sel = np.ones(len(U), dtype=bool) if only is None else only
    if np.any(np.isnan(ul[sel])):
        fail(what, 'a NaN bound (row %d)', np.argmax(sel & np.any(np.isnan(ul), axis=1)))
    dead = sel & ~live
    if np.any(dead & ~((ul[:, 0] == -np.inf) & (ul[:, 1] == -np.inf))):
        fail(what, 'a dead row without U = L = -inf (row %d)', np.argmax(dead & ~((ul[:, 0] == -np.inf) & (ul[:, 1] == -np.inf))))
    whole = (ul[:, 0] == np.inf) & (ul[:, 1] == -np.inf)
    coded_unc = bad | ((mir['code'] == M.I4_UNCERTAIN) if 'code' in mir else np.zeros(len(U), dtype=bool))
    must = sel & live & (coded_unc | bool(doc['vbad']))
    if np.any(must & ~whole):
        fail(what, 'a NaN row or a bad vector without [-inf, +inf] (row %d)', np.argmax(must & ~whole))
    fin = sel & live & ~must
    unc = fin & whole
    if np.any(unc & ~(doc['c'] <= LD(1e-3) * (1 + LD(1e-2)))):
        i = int(np.argmax(unc & ~(doc['c'] <= LD(1e-3) * (1 + LD(1e-2)))))
        fail(what, 'row %d is "uncertain" although c = 1 - (|s1| + delta1)^2 = %.6g is above the 1e-3 band', i, float(doc['c'][i]))
    fin = fin & ~whole
    if np.any(fin & ~np.isfinite(ul[:, 0]) | fin & ~np.isfinite(ul[:, 1])):
        fail(what, 'a half-infinite interval (row %d)', np.argmax(fin & ~(np.isfinite(ul[:, 0]) & np.isfinite(ul[:, 1]))))
    if np.any(fin & (doc['c'] < LD(1e-3) * (1 - LD(1e-2)))):
        fail(what, 'a finite interval although c is below the 1e-3 band (row %d)', np.argmax(fin & (doc['c'] < LD(1e-3) * (1 - LD(1e-2)))))
    stats = dict(rows=int(fin.sum()), uncertain=int(unc.sum()), worst=0., attain={})
    if not np.any(fin):
        return stats
    with np.errstate(all='ignore'):
        hwid = (U - L) / 2
        centre = (U + L) / 2
    with np.errstate(all='ignore'):
        out = np.where(fin, np.maximum(L - allow - f, f - (U + allow)), -np.inf)      # > 0: violated
        ratio = np.where(fin, np.maximum(L - f, f - U) / hwid, -np.inf)
    stats['worst'] = float(np.max(ratio)) + 1.            # |centre - f| / half-width of the row nearest to (or past) an end
    smallest = np.min(hwid[fin])
    if not np.max(allow[fin]) < LD(1e-3) * smallest:
        fail(what, "the fp64 kernel's allowance %.3g is not below 1e-3 of the smallest half-width %.3g", float(np.max(allow[fin])), float(smallest))
    if np.any(out > 0):
        i = int(np.argmax(out))
        fail(what, 'row %d: the exact score %.12g is outside [L, U] = [%.9g, %.9g] by %.3g half-widths (%d rows)', i, float(f[i]), float(L[i]),
             float(U[i]), float(out[i] / hwid[i]), int(np.sum(out > 0)))
    # fp32 evaluation: relative 1e-4 plus 1e-6 (1 + |f|); and c = 1 - a * a itself is formed in fp32 with an absolute error
    # <= 3 * 2^-24 (the sum a, its square, the difference: bc_prefilter_i8.h says as much), which the c^(-3/2) of the slope term
    # turns into a relative 1.5 * 3 * 2^-24 / c -- 1.3e-4 at c = 2e-3, where the first two terms alone would fail a sound bound
    with np.errstate(all='ignore'):
        tol = (LD(1e-4) + LD(4.5) * LD(2) ** -24 / np.where(doc['c'] > 0, doc['c'], 1)) * doc['e'] + LD(1e-6) * (1 + np.abs(f))
    off = np.where(fin, np.abs(hwid - doc['e']) - tol, -np.inf)
    if np.any(off > 0):
        i = int(np.argmax(off))
        fail(what, 'row %d: half-width %.9g differs from the documented formula %.9g (c = %.4g)', i, float(hwid[i]), float(doc['e'][i]), float(doc['c'][i]))
    offc = np.where(fin, np.abs(centre - doc['f']) - tol, -np.inf)
    if np.any(offc > 0):
        i = int(np.argmax(offc))
        fail(what, 'row %d: centre %.9g differs from the score of the stored digits %.9g', i, float(centre[i]), float(doc['f'][i]))
    stats['f'] = f
    stats['fin'] = fin
    stats['attain_rows'] = np.where(fin, np.abs(centre - f) / hwid, 0).astype(np.float64)
    return stats


def check_theta0(s, mir):
    f, allow, _ = s['_exact'] if '_exact' in s else exact_scores(s, mir['u'])
    ok = mir['live'] & ~mir['bad'] & np.isfinite(f.astype(np.float64))
    if not np.any(ok):
        return
    top = np.max(f[ok] + allow[ok])
    th = np.asarray(s.theta0, dtype=np.float32)
    if np.any(np.isnan(th)) or np.any(th.astype(LD) > top):
        b = int(np.argmax(np.isnan(th) | (th.astype(LD) > top)))
        fail('theta0', 'block %d: theta0 = %.9g is above the best exact score %.9g', b, float(th[b]), float(top))


def check_all(s, skip=(), memo=None):
    """Every link the snapshot has the buffers for.  Returns {level: stats}.  memo: a dict the caller keeps while the MIRRORS
    stay the same (one matrix, many vectors): they are then decoded and checked once."""
    out = {}
    memo = {} if memo is None else memo
    two = s.get('two', False)
    if 'm8' not in memo:
        memo['m8'] = check_mirror_i8(s) if 'mirror' not in skip else _decoded_i8(s)
        if two:
            memo['m4'] = check_mirror_i4(s) if 'mirror' not in skip else _decoded_i4(s)
            if 'mirror' not in skip:
                check_r8(s)
    m8, m4 = memo['m8'], memo.get('m4')
    s['_exact'] = exact_scores(s, m8['u'])
    if 'record' not in skip:
        check_record(s, 'i8')
        if two:
            check_record(s, 'i4')
    if s.get('ul_i8') is not None:
        out['i8'] = check_intervals(s, s.ul_i8, 'i8', m8, False, 'int8 interval')
    if two and s.get('ul_i4') is not None:
        out['i4'] = check_intervals(s, s.ul_i4, 'i4', m4, True, '4-bit interval')
    if two and s.get('ul8') is not None:
        done = ~np.isnan(s.ul8[:, 0]) | ~np.isnan(s.ul8[:, 1])
        out['l2'] = check_intervals(s, s.ul8, 'i8', m8, False, 'level 2 interval', only=done)
        check_theta0(s, m8)
        # level 1 passes on every row whose upper bound reaches theta >= theta0, never a dead one
        if np.any(done & ~m8['live']):
            fail('level 2', 'a dead row was re-bounded')
    return out


def _decoded_i8(s):
    u, live, bad = unit_rows(s)
    rq = s.rowq.view(np.float16).reshape(-1, 2)
    return dict(u=u, live=live, bad=bad, q=decode_i8(s), scale=rq[:, 0].astype(LD), delta=rq[:, 1].astype(LD))


def _decoded_i4(s):
    u, live, bad = unit_rows(s)
    code = s.rowq4.astype(np.int64)
    return dict(u=u, live=live, bad=bad, q=decode_i4(s), scale=(code & 0xff).astype(LD) / 1024, delta=(code >> 8).astype(LD) / 512, code=code >> 8)


# ------------------------------------------------------------------ the case matrices and vectors
def correlated(rng, n, s):
    base = rng.randn(n, 12).dot(rng.randn(12, s)) + 0.3 * rng.randn(n, s)
    return base - base.mean(axis=1)[:, None]


def _four_squares(T, centre):
    """four integers in 0 .. 127 whose squares sum to T, near `centre` where possible"""
    for width in (6, 14):
        lo, hi = max(0, centre - width), min(127, centre + width)
        for a in range(lo, hi + 1):
            for b in range(a, hi + 1):
                for c in range(b, hi + 1):
                    d2 = T - a * a - b * b - c * c
                    if d2 < 0:
                        break
                    d = isqrt(d2)
                    if d * d == d2 and d <= 127:
                        return [a, b, c, d]
    return None


@functools.lru_cache(maxsize=None)
def exact_row(S):
    """Integer entries |q_k| <= 127 (q_0 = 127), nearly equal, with sum q_k^2 = N just above 1 / h^2 for a half h: the int8
    mirror of the row q / ||q|| has scale h and delta ~ 1 / (2 N).  Returns (q, h)."""
    assert S >= 8
    best = None
    for p in range(10, 26):
        for m in range(1024, 2048):
            inv2 = Fraction(1 << (2 * p), m * m)           # 1 / h^2 for h = m / 2^p
            if not (S * 110 ** 2 <= inv2 <= S * 127 ** 2):
                continue
            N = -(-inv2.numerator // inv2.denominator)
            if N > S * 125 ** 2 or N == inv2:
                continue
            eps = float(N - inv2) / N
            key = (N < S * 122 ** 2, eps)
            if best is None or key < best[0]:
                best = (key, N, Fraction(m, 1 << p))
    _, N, h = best
    rest, uni = N - 127 ** 2, S - 5
    base = isqrt(rest // (S - 1))
    rng = np.random.RandomState(S)
    for _ in range(400):                                   # S - 5 entries near the mean, four that make the sum exact
        mid = [int(x) for x in rng.randint(max(1, base - 2), min(127, base + 3) + 1, size=uni)]
        T = rest - sum(x * x for x in mid)
        for _ in range(20000):                             # steer the remainder towards four entries near the mean
            if T > 4 * (base - 1) ** 2 and uni:
                k = rng.randint(uni)
                if mid[k] < 127:
                    T -= 2 * mid[k] + 1
                    mid[k] += 1
            elif T < 4 * (base - 8) ** 2 and uni:
                k = rng.randint(uni)
                if mid[k] > 1:
                    T += 2 * mid[k] - 1
                    mid[k] -= 1
            else:
                break
        if T < 0 or T > 4 * 126 ** 2:
            continue
        four = _four_squares(T, isqrt(T // 4))
        if four is not None and min(four) >= base - 25:
            q = [127] + mid + four
            assert len(q) == S and sum(x * x for x in q) == N and max(q) == 127
            return np.array(q, dtype=np.int64), float(h)
    raise AssertionError('no exact row for S = %d' % S)


LADDER = [0.80, 0.84, 0.87, 0.89, 0.91, 0.93, 0.95, 0.97, 0.98, 0.985, 0.988, 0.990, 0.992, 0.994, 0.996, 0.998, 0.9995]
ROW_EXACT, ROW_LADDER, ROW_PARALLEL, ROW_ZERO, ROW_NAN, ROW_INF = 3, 10, 40, 50, 51, 52
ROWS_E = [5, 63]                   # rows whose own quantisation error the `row` vectors follow (n >= 64)


def signs_of(S):
    return np.where(np.random.RandomState(900 + S).rand(S) < 0.5, -1., 1.)


def slope_vectors(S):
    """(v0, v1) of the `slope` case, interleaved; v1 alone is what the ladder rows are built around."""
    q, _ = exact_row(S)
    sg = signs_of(S)
    u = sg * q / np.sqrt(float(np.sum(q * q)))
    T = np.where(np.arange(S) % 4 != 3, 126., -126.)           # three in four positive: s1 ~ 0.5
    x = sg * (T + 0.4999 * q / 127.)
    x[0] = sg[0] * 127.
    v1 = x / np.sqrt(np.sum(x * x))
    v0 = u / np.sqrt(np.sum(u * u))
    return np.stack((v0, v1), axis=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def case_phi(S, n):
    """The case matrix: correlated rows and, from 64 rows and S >= 8, the special rows named above."""
    rng = np.random.RandomState(31 * S + n)
    phi = correlated(rng, n, S) if S > 1 else rng.randn(n, 1)
    if n >= 64 and S >= 8:
        q, _ = exact_row(S)
        phi[ROW_EXACT] = signs_of(S) * q                       # (integers: the device's norm is sqrt(N), u = q / sqrt(N))
        v1 = slope_vectors(S)[1::2]
        for j, al in enumerate(LADDER):
            w = rng.randn(S)
            w -= w.dot(v1) * v1
            w /= np.linalg.norm(w)
            phi[ROW_LADDER + j] = (al * v1 + np.sqrt(1. - al * al) * w) * (0.5 + rng.rand())
        phi[ROW_PARALLEL] = 3.7 * v1
        phi[ROW_ZERO] = 0.
        phi[ROW_NAN] = phi[ROW_NAN - 10]
        phi[ROW_NAN, S // 2] = np.nan
        phi[ROW_INF] = phi[ROW_INF - 10]
        phi[ROW_INF, 0] = np.inf
    phi.setflags(write=False)
    return phi


def finite_b(phi):
    """A right-hand side for a solver over a case matrix (the sum of its finite rows)."""
    ok = np.all(np.isfinite(phi), axis=1)
    return phi[ok].sum(axis=0)


@functools.lru_cache(maxsize=None)
def model_mirrors(S, n):
    phi = case_phi(S, n)
    s = M.run_model(phi, 1, np.ones(S), two_level=True)
    return s


def case_vectors(S, n):
    """[(name, mode, v, post_div, targeted term, targeted row or None)] for the case matrix (S, n)."""
    phi = case_phi(S, n)
    rng = np.random.RandomState(77 * S + n)
    out = []
    r = rng.randn(S) * 2.5
    out.append(('random', 1, r, 1.0, None, None))
    out.append(('random-pd', 1, rng.randn(S), -2.5, None, None))
    g = rng.randn(S, 2)
    g /= np.linalg.norm(g, axis=0)
    out.append(('random-giga', 0, g.reshape(-1).copy(), 1.0, None, None))
    out.append(('scaled', 1, 0.01 * r, 1.0, None, None))               # (the vectors of the step before: r -- theta0 must follow)
    special = n >= 64 and S >= 8
    mm = model_mirrors(S, n)
    m8 = _decoded_i8(mm)
    for i in (ROWS_E if special else [0]):
        if i >= n:
            continue
        e = (m8['q'][i, :S].astype(LD) * m8['scale'][i] - m8['u'][i]).astype(np.float64)
        if np.linalg.norm(e) > 0:
            out.append(('row8:%d' % i, 1, 3. * e / np.linalg.norm(e), 1.0, 'row', i))
        if mm.two:
            m4 = _decoded_i4(mm)
            e4 = (m4['q'][i, :S].astype(LD) * m4['scale'][i] - m4['u'][i]).astype(np.float64)
            if np.linalg.norm(e4) > 0:
                out.append(('row4:%d' % i, 1, 3. * e4 / np.linalg.norm(e4), 1.0, 'row4', i))
    if special:
        q, _ = exact_row(S)
        sg = signs_of(S)
        vstep = 2. ** -14
        Q = rng.randint(0, 2000, size=S).astype(np.float64)
        v = sg * (Q + 0.4999 * q / 127.) * vstep
        v[0] = sg[0] * 16256. * vstep
        out.append(('vec', 1, v, 1.0, 'vec', ROW_EXACT))
        out.append(('slope', 0, slope_vectors(S), 1.0, 'slope', ROW_EXACT))
        bad = rng.randn(S)
        bad[S // 3] = np.nan
        out.append(('nan-v', 1, bad, 1.0, None, None))
    return out


def case_list():
    """(S, n) of every case matrix: the 21 classes of the two-level sweep and their edges at the default size, the S at which the
    int8 builders and forms change, and the sizes around one and two mirror tiles."""
    cases = [(S, 3001) for S in S_LIST] + [(S, 300) for S in EXTRA_S]
    cases += [(37, n) for n in N_LIST if n not in (300, 3001)] + [(8, n) for n in (1, 257)]
    return cases


def previous_vector(S, n):
    """The `scaled` case's vectors of the step before, and the seeds they leave: the 32 best rows under them."""
    vecs = dict((name, v) for name, _, v, _, _, _ in case_vectors(S, n))
    r = vecs['random']
    phi = case_phi(S, n)
    with np.errstate(all='ignore'):
        sc = phi.dot(r) / np.sqrt(np.sum(phi * phi, axis=1))
    sc = np.where(np.isfinite(sc), sc, -np.inf)
    return r, np.argsort(-sc)[:32]
