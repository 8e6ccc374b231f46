"""The case tables of the strided resampling egress tests (fvad_egress_resample_strided*; test_egress_strided_host.py,
test_egress_strided_gpu.py), built on egress_resample_cases (`er`) and ingest_resample_cases (`rc`).

A strided table is an er.case_table re-laid: the rows (but for src_offset), the `data` and therefore the float64 model are the
same; each row's data sits `step` apart in its lanes from a src_offset that runs through the 4 alignments, and EVERY other lane
sample is NaN -- the samples between two of the stride as well as those around a row.  A NaN in the output shows an off-stride
sample that reached a sum.  `compacted` lays the same rows out contiguously again: the lanes fvad_egress_resample would be given
for them, so the parent's kernel is the yardstick for the bytes.

`check_model` is fvad_egress_resample_strided_check restated in python integers (no width to get wrong)."""
import numpy as np

import egress_resample_cases as er
import ingest_resample_cases as rc

OK, INVALID, RANGE = 0, -100, -6
STEP_MAX = 16
UP_MAX, TAPS_MAX = 640, 20481


def lagged(taps, lag):
    """taps' = [0] * 2 lag + taps: the centre moves from K to K + lag, so output o sits at fine index o down - lag"""
    return np.concatenate([np.zeros(2 * lag, np.float32), np.asarray(taps, np.float32)])


def _taps(up, down, spec):
    kind, arg = spec
    if kind == "lagged":                      # the default design, lagged
        return lagged(rc.design(up, down, 16).astype(np.float32), arg)
    if kind == "one":
        return np.array([1.0], np.float32)
    return rc.case_taps(up, down, arg, kind)   # "noise" / "design" with a half


# (up, down, taps, step): 48 kHz and 16 kHz recordings of a 16 kHz stream 3 apart, 44.1 kHz with the table in global memory
# (14701 taps), asymmetric taps at steps 2 and 16, and step 1 (the parent's bytes over the same lanes)
CASES = ((3, 1, ("lagged", 2), 3), (1, 1, ("one", 0), 3), (441, 160, ("lagged", 294), 3), (7, 5, ("noise", 2), 2), (2, 1, ("noise", 3), 16),
         (147, 160, ("design", 16), 1))


def case_id(c):
    return f"{c[0]}-{c[1]}-step{c[3]}"


def case_taps(c):
    return _taps(c[0], c[1], c[2])


def _lay(table, step, k0):
    """the table's rows laid `step` apart: rows of one first_lane one behind the other, src_offset through the 4 alignments from
    k0 on, NaN everywhere else; lane_stride odd"""
    rows = table["rows"].copy()
    cur = {}
    for i, (_, _, C, _, l0, _, _, nf, _, _) in enumerate(rows.tolist()):
        c = cur.get(l0, 0)
        src = c + 1 + (k0 + i - (c + 1)) % 4
        rows[i, 5] = src
        cur[l0] = src + ((nf - 1) * step + 1 if nf else 0)
    n_samples = max(cur.values()) + 2
    lane_stride = n_samples + 1 + (n_samples % 2)
    lanes = np.full((table["n_lanes"], lane_stride), np.nan, np.float32)
    for (_, _, C, _, l0, src, _, nf, _, _), v in zip(rows.tolist(), table["data"]):
        if nf:
            lanes[l0:l0 + C, src:src + (nf - 1) * step + 1:step] = v.T
    return dict(table, rows=rows, lanes=lanes, lane_stride=lane_stride, n_samples=n_samples, step=step)


def strided(table, step, seed=0):
    """an er.case_table re-laid `step` apart (the module's docstring); the seed picks the first alignment"""
    return _lay(table, step, int(np.random.default_rng(seed).integers(4)))


def compacted(table):
    """the same rows over contiguous lanes: what fvad_egress_resample would be given"""
    return _lay(table, 1, 1)


def twin_f32(table):
    """er.twin_f32 of a strided table (the lanes and the step stay)"""
    return er.twin_f32(table)


def check_model(rows, out_bytes, up, down, taps, step, src_format, n_lanes, lane_stride, n_samples):
    """fvad_egress_resample_strided_check in python integers; taps: None or a float array"""
    if src_format != 0:
        return INVALID
    if not (1 <= up <= UP_MAX and down >= 1):
        return INVALID
    if not 1 <= step <= STEP_MAX:
        return INVALID
    if taps is None or len(taps) == 0 or len(taps) % 2 == 0 or len(taps) > TAPS_MAX or not np.isfinite(np.asarray(taps, np.float64)).all():
        return INVALID
    n_taps = len(taps)
    if len(rows) == 0:
        return OK
    if n_lanes > 1 and lane_stride < n_samples:
        return INVALID
    for at, n_out, C, fmt, l0, src, fb, nf, sf, out_from in rows:
        if fmt not in (er.F32, er.PCM16, er.PCM24) or not 1 <= C <= 64:
            return INVALID
        if sf * up >= 1 << 62:
            return INVALID
        if out_from + n_out >= 1 << 64 or out_from + n_out > min(rc.out_frames(sf, up, down), (1 << 64) - 1):
            return INVALID
        if fb + nf >= 1 << 64 or fb + nf > sf:
            return INVALID
        lo, hi = rc.window(up, down, n_taps, sf, out_from, n_out)
        if hi > lo and (fb > lo or fb + nf < hi):
            return INVALID
        if er.tile(up, down, n_taps, C, fmt) == 0:
            return INVALID
    for at, n_out, C, fmt, l0, src, fb, nf, sf, out_from in rows:
        if l0 >= n_lanes or C > n_lanes - l0:
            return RANGE
        if nf and src + (nf - 1) * step + 1 > n_samples:
            return RANGE
        if at + n_out * C * er.SAMPLE_BYTES[fmt] > out_bytes:
            return RANGE
    ranges = sorted((r[0], r[0] + r[1] * r[2] * er.SAMPLE_BYTES[r[3]]) for r in rows if r[1])
    for (_, to), (frm, _) in zip(ranges[:-1], ranges[1:]):
        if frm < to:
            return INVALID
    return OK


# ---------------------------------------------------------------- the harness's filter, restated
def network_filter(rate, design=rc.design):
    """run_denoise(source="network")'s filter for a file at `rate`, by the rule: -> dict(up, down, lag, lead, n_taps) or None
    where the harness refuses (no ratio with up <= 640, or a lagged design longer than TAPS_MAX)"""
    from math import gcd
    g = gcd(rate, 16000)
    up, down = rate // g, 16000 // g
    if up > UP_MAX:
        return None
    if rate == 16000:
        return dict(up=1, down=1, lag=0, lead=2, n_taps=1)
    lag = 2 * up // 3 if up % 3 == 0 else 0
    n_taps = 2 * 16 * max(up, down) + 1 + 2 * lag
    if n_taps > TAPS_MAX:
        return None
    return dict(up=up, down=down, lag=lag, lead=0 if up % 3 == 0 else 2, n_taps=n_taps)
