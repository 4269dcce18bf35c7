"""Edge corpus shared by the CPU (restatement vs reference) and GPU (HIP engine vs reference) suites: every node type at its
clamps, at the edges of its domain and with non-finite samples — the inputs `cases.NODE_CASES` stays away from.

Every edge parameter appears once as a constant and once as a signal (`S(v)`: the same value carried by a frame-rate buffer),
because the kernels choose their code by constness (run_svf_coef's constF / constQ / constAll, ser_phasor's v_fract form, the
merged OP_PHASE task, run_delay's block minimum).

What is kept OUT, because the reference does not define it: NaN, infinity or a value outside `int` on an input from which a node
computes an address or an integer — a `delay` length (Delays.h:130), a `table` index (Table.h:61), a `sample` rate or offset,
`sampleseq`'s time, `seq` / `seq2` offsets. Finite out-of-range values go to the delay length and the table index only, which
the reference clamps (Delays.h:109, Table.h:60)."""
import numpy as np

from elementary_amd import el
from helpers import lcg_noise

TOL = 1e-6
X = lambda ch=0: el.in_({"channel": ch})  # noqa: E731


def S(v, ch=0):
    """The constant `v` as a signal: v + 0 * x is v in every frame (v + (+-0) == v, and 0 + -0 == +0), but no engine sees a
    constant operand."""
    return el.add(float(v), el.mul(0.0, X(ch)))


def edge_inputs(k, block):
    """Block k of the four input channels, [4, block] float32: 0 and 1 the usual amplitude-0.5 LCG noise (cases.py seeds);
    2 = channel 0 with +0.0 in every 7th frame and -0.0 in every 11th (from frame 3); 3 = amplitude-8 noise rounded to quarter
    steps (integers, .5 ties, and 2 * x3 has a tie in every other step)."""
    x0, x1 = lcg_noise(block, 1 + 97 * k, 0.5), lcg_noise(block, 2 + 97 * k, 0.5)
    x2 = x0.copy()
    x2[::7] = 0.0
    x2[3::11] = -0.0
    x3 = (np.round(lcg_noise(block, 3 + 97 * k, 8.0).astype(np.float64) * 4.0) / 4.0).astype(np.float32)
    return np.stack([x0, x1, x2, x3])


def edge_resources():
    from cases import node_case_resources
    return node_case_resources()          # /t/ramp, /t/five, /t/one (and /t/stereo for mc.table)


def _both(f, *vals):
    """f(v) for every v as a constant, then as a signal."""
    return [f(v) for v in vals] + [f(S(v)) for v in vals]


# ---- phase recurrences ------------------------------------------------------------------------------------------------------
def _phasor_edges(n, first=0):
    # -0.001 Hz: the step is -2.3e-8, `next - floor(next)` rounds to exactly 1.0 and the reference outputs it (Core.h:85-136);
    # 0 and 50 000 Hz keep the constant non-negative form (v_fract), the negative ones and every signal the general one
    return (_both(el.phasor, -440.0, -0.001, 0.0, 50000.0) + [el.phasor(el.mul(3000.0, X(0)))]
            + [el.syncphasor(-440.0, el.train(37.0)), el.syncphasor(S(-440.0), el.train(37.0)),
               el.syncphasor(el.mul(3000.0, X(0)), el.train(37.0))])


def _blep_edges(n, first=0):
    # 0 Hz: inc == 0 (no correction branch, 0 / 0 never evaluated); negative: the phase only ever wraps at >= 1 (Oscillators.h),
    # so it runs off below 0 and the correction grows; 30 000 Hz: inc in (0.5, 1), both correction branches overlap
    out = []
    for osc in (el.blepsaw, el.blepsquare, el.bleptriangle):
        out += _both(osc, -440.0, 0.0, 30000.0) + [osc(el.mul(30000.0, X(0)))]
    return out


# ---- double-state filters at their clamps -----------------------------------------------------------------------------------
CUTOFFS = (5.0, -100.0, 20.0, 30000.0, 1.0e6)       # below, far below, at the lower clamp; above sr/2.0001 at 44.1 / 48 kHz; above at any rate
QS = (0.01, 0.25, 20.0, 100.0, -1.0)


def _svf_clamps(n, first=0):
    out = []
    for f in (el.lowpass, el.highpass, el.bandpass, el.notch, el.allpass):
        out += _both(lambda fc: f(fc, 1.0, X(0)), *CUTOFFS) + [f(el.mul(60000.0, X(1)), 1.0, X(0))]
        out += _both(lambda q: f(1000.0, q, X(0)), *QS) + [f(1000.0, el.mul(60.0, X(1)), X(0))]
    # both clamps at once, constAll and neither
    out += [el.lowpass(1.0e6, 100.0, X(0)), el.lowpass(S(1.0e6), S(100.0), X(0)), el.lowpass(5.0, 0.01, X(0)), el.lowpass(S(5.0), S(0.01), X(0))]
    return out


def _shelf_clamps(n, first=0):
    out = []
    for f in (el.lowshelf, el.highshelf, el.peak):
        out += _both(lambda fc: f(fc, 1.0, 6.0, X(0)), *CUTOFFS) + [f(el.mul(60000.0, X(1)), 1.0, 6.0, X(0))]
        out += _both(lambda q: f(1000.0, q, 6.0, X(0)), *QS) + [f(1000.0, el.mul(60.0, X(1)), 6.0, X(0))]
        out += _both(lambda g: f(1000.0, 1.0, g, X(0)), 40.0, -40.0) + [f(1000.0, 1.0, el.mul(80.0, X(1)), X(0))]
    return out


def _mm1p_clamps(n, first=0):
    out = []
    for mode in ("lowpass", "highpass", "allpass"):
        f = lambda g: el.mm1p({"mode": mode}, g, X(0))  # noqa: E731
        out += _both(f, -0.5, 0.0, 0.9999, 5.0) + [f(el.mul(3.0, X(1))), f(el.prewarp(30000.0)), f(el.prewarp(S(30000.0)))]
    return out


# ---- delay: the threshold between the sample-parallel branch and the serial walk ------------------------------------------------
def delay_ramp(n):
    return el.add(n - 28.0, el.mul(15.0 / n, el.mod(el.time(), 4.0 * n)))


def _delay_threshold(n, first=0):
    """Every length is finite. run_delay (island_ops.inc) clamps it with clampf(len, 0, size) before any use — the block minimum,
    the parallel branch and the serial walk each clamp on their own line — so offset is in [0, size], readFrac =
    float(size + w) - offset is in [w, size + w] with 0 <= w < size, readLeft in [0, 2 size), readRight <= 2 size, and both are
    taken `% size` (Delays.h:109, 129-139: the same clamp and the same modulo). Writes go to w < size. Feedback is a value, never
    an index. The parallel branch runs when min(offset) >= n + 2 and size >= n: lengths n .. n + 1.5 stay serial, n + 2 and
    n + 2.5 go parallel; n + 2 + 60 x1 has its minimum below the threshold in practically every block (the serial walk at lengths
    around it), and a ramp over 4 blocks, n - 28 + (15 / n) (t mod 4 n), stays below n + 2 for two blocks and at or above it for
    the next two: the branch changes from block to block inside one stream."""
    size = 4 * n
    d = lambda length, fb=0.5, sz=size: el.delay({"size": sz}, length, fb, X(0))  # noqa: E731
    out = _both(d, float(n), n + 1.0, n + 1.5, n + 2.0, n + 2.5, float(size), 2.5 * size)
    out += [d(el.add(n + 2.0, el.mul(60.0, X(1)))), d(delay_ramp(n))]
    out += _both(lambda fb: d(n + 2.5, fb), 1.5, -3.0) + [d(n + 2.5, el.mul(4.0, X(1)))]          # parallel branch, clamped feedback
    out += _both(lambda fb: d(10.25, fb), 1.5, -3.0) + [d(10.25, el.mul(4.0, X(1)))]             # serial walk, clamped feedback
    out += [d(el.mul(400.0, X(1))), d(el.mul(400.0, X(1)), 0.9, 64)]                            # negative -> 0: the offset <= eps bypass; > size
    small = max(4, n // 3)                                                                         # size < n: always serial, several wraps a block
    out += [d(small - 0.5, 0.5, small), d(S(float(small)), -0.7, small), d(el.mul(400.0, X(1)), 0.5, small)]
    return out


# ---- table: the index clamp ------------------------------------------------------------------------------------------------
def _table_clamps(n, first=0):
    """The index is finite; run_table clamps it with clampf(x, 0, 1) and scales by size - 1: readLeft in [0, size - 1], readRight
    <= size, both `% size` (Table.h:60-66). /t/one has size 1: readPos == 0, readRight % 1 == 0."""
    idx = el.mul(4.0, X(0))                                                                       # [-2, 2]
    return [el.table({"path": p}, idx) for p in ("/t/ramp", "/t/five", "/t/one")] + _both(lambda v: el.table({"path": "/t/five"}, v), -2.0, 3.0, 1.0, 0.0)


def _table_clamps_mc(n, first=0):
    """mc.table is the same kernel body with one buffer per channel (reference only: the restatement has no mc nodes)."""
    return el.mc.table({"path": "/t/stereo", "channels": 2}, el.mul(4.0, X(0))) + el.mc.table({"path": "/t/stereo", "channels": 2}, 3.0)


# ---- stateless math at the edges of its domain -------------------------------------------------------------------------------
def _math_domain(n, first=0):
    x0, x1, x2, x3 = X(0), X(1), X(2), X(3)
    out = [f(a) for f in (el.ln, el.log, el.log2, el.sqrt) for a in (x0, x2, el.abs(x2))]            # negatives -> NaN, +-0 -> -inf / +-0
    out += [el.div(x0, x2), el.mod(x0, x2), el.mod(x3, 0.75), el.mod(x3, S(0.75)), el.div(x0, 0.0), el.div(x0, S(0.0))]
    out += [el.pow(x0, x1), el.pow(x2, -1.0), el.pow(x2, S(-1.0)), el.pow(x3, x3), el.pow(x0, 2.0), el.pow(x0, S(2.0)), el.pow(x2, -0.5)]
    out += [f(a) for f in (el.round, el.ceil, el.floor) for a in (x3, el.mul(2.0, x3))]
    out += [el.exp(el.mul(400.0, x0)), el.tanh(el.mul(1.0e6, x0)), el.tan(el.mul(3.2, x0)), el.asinh(el.mul(1.0e30, x0))]
    return out


def _nan_ordering(n, first=0):
    """N is NaN where x1 < 0, I is +inf where x0 > 0.222 (and merely large or tiny elsewhere). std::min(a, b) is (b < a) ? b : a:
    with a NaN on either side the FIRST operand comes back, and a fold carries that on (Math.h:59-89)."""
    x0, x1 = X(0), X(1)
    N, I = el.ln(x1), el.exp(el.mul(400.0, x0))  # noqa: E741
    out = [el.min(x0, N), el.min(N, x0), el.max(x0, N), el.max(N, x0)]
    for f in (el.min, el.max):
        out += [f(N, x0, 0.1), f(x0, N, 0.1), f(x0, 0.1, N), f(I, x0, N), f(N, I, x0)]
    for f in (el.le, el.leq, el.ge, el.geq, el.eq, el.and_, el.or_):
        out += [f(N, x0), f(x0, N), f(I, x0), f(x0, I), f(N, I), f(I, N)]
    out += [el.eq(I, I), el.eq(N, N), el.add(I, el.mul(-1.0, I)), el.mul(I, 0.0), el.mul(I, S(0.0)), el.sub(I, I), el.sub(0.0, I)]
    return out


# ---- non-finite samples into recurrences, scans and rings ------------------------------------------------------------------------
def nonfinite_signal(n, first=0):
    """x0, bit for bit, except: +inf in frame 7 of block 2, -inf in frame 3 of block 4, NaN from 3 frames before the end of block 5
    to frame 4 of block 6 (an island across a block boundary); blocks counted from block `first`. The three gates are exact 0 / 1 signals of el.time() (integers
    below 2^24); exp(1000 g) - 1 is 0 or +inf, ln(1 - 2 g) is 0 or NaN — expf(0) == 1 and logf(1) == 0 in every libm."""
    t = el.sub(el.time(), float(first * n))
    gp, gm = el.eq(t, 2.0 * n + 7.0), el.eq(t, 4.0 * n + 3.0)
    gn = el.mul(el.geq(t, 6.0 * n - 3.0), el.leq(t, 6.0 * n + 4.0))
    pinf = el.sub(el.exp(el.mul(1000.0, gp)), 1.0)
    ninf = el.sub(1.0, el.exp(el.mul(1000.0, gm)))
    nan = el.ln(el.sub(1.0, el.mul(2.0, gn)))
    return el.add(X(0), pinf, ninf, nan)


NONFINITE_BIT_EXACT = (0, 1, 2, 3, 4, 5, 6)        # roots of nonfinite_into_state held bit for bit where finite: s, pole x2, biquad, z, zero, sdelay


def _nonfinite_into_state(n, first=0):
    """`delay` takes s as x ONLY (its length is an address). latch, accum, maxhold and counter compare or add s, none indexes by it."""
    s = nonfinite_signal(n, first)
    return [s, el.pole(0.99, s), el.pole(S(0.99), s), el.biquad(0.2, 0.3, 0.2, -0.5, 0.2, s), el.z(s), el.zero(0.5, 0.5, s),
            el.sdelay({"size": 10}, s),
            el.env(el.tau2pole(0.001), el.tau2pole(0.05), s), el.lowpass(800.0, 1.0, s), el.lowpass(S(800.0), 1.0, s),
            el.highshelf(4000.0, 0.7, -4.5, s), el.mm1p({"mode": "lowpass"}, 0.3, s),
            el.delay({"size": 100}, 10.25, 0.5, s), el.delay({"size": 4 * n}, n + 2.5, 0.5, s),
            el.latch(el.train(100.0), s), el.latch(s, X(1)), el.accum(s, el.train(20.0)), el.accum(X(1), s),
            el.maxhold({"hold": 3.0}, s, el.train(9.0)), el.maxhold({}, X(1), s), el.counter(s), el.smooth(0.95, s), el.dcblock(s)]


# ---- the clock far from zero --------------------------------------------------------------------------------------------------
def clock_starts(block, first=0):
    """sample_time of block 0, such that block `first` + 2 crosses 2^24 (float's integers end), 2^31 and 2^32 (32-bit counters);
    and one far beyond."""
    return [2 ** 24 - (first + 2) * block, 2 ** 31 - (first + 2) * block, 2 ** 32 - (first + 2) * block, 2 ** 40 + 3]


def _clock_far_out(n, first=0):
    """sparseq2's time input is finite and only ever compared (SparSeq2.h:98-125; run_sparseq2: a binary search over the event
    times, the index is the search's own counter)."""
    seq = [{"time": float(t), "value": v} for t, v in ((100, 1.0), (2 ** 24 - n, 2.5), (2 ** 24 + n, -1.0), (2 ** 31, 3.0), (2 ** 32 + 7, -2.0), (2 ** 40 + n, 0.5))]
    return [el.mul(2.0 ** -20, el.time()), el.time(), el.metro({"interval": 3.0}), el.metro({"interval": 0.7}),
            el.sparseq2({"seq": seq}, el.time()), el.sparseq2({"seq": seq, "interpolate": 1}, el.time()), el.train(50.0)]


_GROUPS = {
    # name: (roots_fn(n, first), n_in); n = the block size in use (delay_threshold, nonfinite_into_state and clock_far_out depend
    # on it), first = the block the timed events of nonfinite_into_state count from
    "phasor_edges": (_phasor_edges, 4),
    "blep_edges": (_blep_edges, 4),
    "svf_clamps": (_svf_clamps, 4),
    "shelf_clamps": (_shelf_clamps, 4),
    "mm1p_clamps": (_mm1p_clamps, 4),
    "delay_threshold": (_delay_threshold, 4),
    "table_clamps": (_table_clamps, 4),
    "table_clamps_mc": (_table_clamps_mc, 4),
    "math_domain": (_math_domain, 4),
    "nan_ordering": (_nan_ordering, 4),
    "nonfinite_into_state": (_nonfinite_into_state, 4),
    "clock_far_out": (_clock_far_out, 4),
}
NODE_EDGE_CASES = {name: ((lambda n=512, first=0, fn=fn: fn(n, first)), n_in) for name, (fn, n_in) in _GROUPS.items()}
EDGE_REF_ONLY = {"table_clamps_mc"}                       # the restatement has no mc nodes (cases.REF_ONLY)
PER_SAMPLE = {"math_domain", "nan_ordering"}              # stateless: 1e-6 * max(1, |ref|) sample by sample
BIT_EXACT = {"phasor_edges": None, "nonfinite_into_state": NONFINITE_BIT_EXACT}      # group -> roots (None: all) held bit for bit where finite


def edge_roots(name, block, first=0):
    return NODE_EDGE_CASES[name][0](block, first)


def settle_blocks(sample_rate, block):
    """Blocks until every root's 20 ms fade-in (Core.h:80) has settled, and one more: the HIP engine renders launch sets only from
    then on, block by block before."""
    return int(np.ceil(0.020 * sample_rate / block)) + 1


def compare_edges(name, got, ref, what=""):
    """Every sample of got / ref [blocks, roots, frames]: NaN where the reference is NaN, the same infinity where it is infinite,
    finite and within tolerance elsewhere — 1e-6 * max(1, |ref|) per sample for the stateless groups, 1e-6 * max(1, max |finite
    ref| of the root) for the others, equal bits (where finite) for the float recurrences of BIT_EXACT. Raises AssertionError
    naming the first failing root, block and frame with both values."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    rnan, rinf = np.isnan(ref), np.isinf(ref)
    bad = (rnan & ~np.isnan(got)) | (rinf & ~(got == ref)) | (fin & ~np.isfinite(got))
    both = fin & np.isfinite(got)
    refz = np.where(fin, ref, 0.0).astype(np.float64)
    if name in PER_SAMPLE:
        tol = TOL * np.maximum(1.0, np.abs(refz))
    else:
        tol = np.broadcast_to(TOL * np.maximum(1.0, np.abs(refz).max(axis=(0, 2)))[None, :, None], ref.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(np.where(both, got, 0.0).astype(np.float64) - refz)
    bad |= both & (err > tol)
    if name in BIT_EXACT:
        roots = BIT_EXACT[name]
        sel = np.zeros(ref.shape, bool)
        sel[:, (slice(None) if roots is None else list(roots)), :] = True
        bad |= sel & both & (got.view(np.uint32) != ref.view(np.uint32))
    if bad.any():
        order = np.argwhere(np.transpose(bad, (1, 0, 2)))[0]                 # first failing root, then its first block / frame
        r, b, f = (int(v) for v in order)
        n_bad = int(bad[:, r, :].sum())
        raise AssertionError(f"{name}{' ' + what if what else ''}: root {r}, block {b}, frame {f}: got {got[b, r, f]!r} "
                             f"(bits {got.view(np.uint32)[b, r, f]:#010x}), reference {ref[b, r, f]!r} (bits {ref.view(np.uint32)[b, r, f]:#010x}), "
                             f"tolerance {float(tol[b, r, f]):.3e}; {n_bad} bad samples in this root, {int(bad.any(axis=(0, 2)).sum())} bad roots "
                             f"{np.flatnonzero(bad.any(axis=(0, 2))).tolist()[:24]}")
