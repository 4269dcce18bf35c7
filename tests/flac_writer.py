"""A small pure-Python FLAC frame writer for building decoder inputs, written from RFC 9639's layout.

It writes what it is told, not what is cheapest: per channel a subframe kind (CONSTANT, VERBATIM, FIXED with an order, LPC with
coefficients, precision and shift), a partition order with one Rice parameter or escape per partition, wasted bits; per frame the
channel assignment, the block size and the frame number. ``elemhip_flac_encode`` never emits LPC, wasted bits or most of these
choices — this does. The corpus of the FLAC input tests is built here (``corpus()``)."""
import numpy as np

import flac_reference as ref

_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
_BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
ASSIGNMENTS = {"independent": None, "left_side": 8, "side_right": 9, "mid_side": 10}


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, nbits, value):
        if nbits:
            self.v = (self.v << nbits) | (int(value) & ((1 << nbits) - 1))
            self.n += nbits

    def unary(self, q):
        self.put(q + 1, 1)

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def utf8_number(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    out = [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(n - 1)][::-1]
    return bytes([((0xFF00 >> n) & 0xFF) | (v >> (6 * (n - 1)))] + out)


def _fits(v, bits):
    return -(1 << (bits - 1)) <= v < (1 << (bits - 1))


def write_subframe(b, samples, bps, kind="VERBATIM", order=0, coefs=None, precision=None, shift=0, porder=0, params=None, wasted=0,
                   method=None, raw_type=None):
    """One subframe into ``b``. ``params``: one entry per partition, a Rice parameter or ``("escape", raw bits)``; default the
    parameter 0 everywhere is rarely wanted — give them. ``raw_type``: a subframe type written as it is (reserved ones)."""
    s = [int(v) for v in samples]
    n = len(s)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in s), "wasted bits need samples that are multiples of 2^wasted"
        s = [v >> wasted for v in s]
        bps -= wasted
    assert all(_fits(v, bps) for v in s), "a sample does not fit the subframe's sample size"
    b.put(1, 0)
    if raw_type is not None:
        b.put(6, raw_type)
    elif kind == "CONSTANT":
        b.put(6, 0)
    elif kind == "VERBATIM":
        b.put(6, 1)
    elif kind == "FIXED":
        b.put(6, 8 + order)
    else:
        order = len(coefs)
        b.put(6, 31 + order)
    if wasted:
        b.put(1, 1)
        b.unary(wasted - 1)
    else:
        b.put(1, 0)
    if raw_type is not None:
        return
    if kind == "CONSTANT":
        assert all(v == s[0] for v in s)
        b.put(bps, s[0])
        return
    if kind == "VERBATIM":
        for v in s:
            b.put(bps, v)
        return
    for v in s[:order]:
        b.put(bps, v)
    if kind == "LPC":
        b.put(4, precision - 1)
        b.put(5, shift)
        for c in coefs:
            assert _fits(c, precision)
            b.put(precision, c)
        res = [s[i] - (sum(coefs[j] * s[i - 1 - j] for j in range(order)) >> shift) for i in range(order, n)]
    else:
        c = _FIXED[order]
        res = [s[i] - sum(c[j] * s[i - 1 - j] for j in range(order)) for i in range(order, n)]
    assert all(_fits(r, 32) and r != -(1 << 31) for r in res), "a residual leaves 32 bits"
    parts = 1 << porder
    assert n % parts == 0 and n // parts >= order
    params = list(params) if params is not None else [0] * parts
    assert len(params) == parts
    if method is None:
        method = 1 if any(not isinstance(p, tuple) and p > 14 for p in params) else 0
    pb = 4 + method
    b.put(2, method)
    b.put(4, porder)
    at = 0
    for p in range(parts):
        cnt = n // parts - (order if p == 0 else 0)
        part = res[at:at + cnt]
        at += cnt
        if isinstance(params[p], tuple):
            raw = params[p][1]
            assert all(raw == 0 and r == 0 or raw and _fits(r, raw) for r in part), "an escaped residual does not fit its raw bits"
            b.put(pb, (1 << pb) - 1)
            b.put(5, raw)
            for r in part:
                b.put(raw, r)
            continue
        k = params[p]
        assert k < (1 << pb) - 1
        b.put(pb, k)
        for r in part:
            u = (r << 1) if r >= 0 else ((-r) << 1) - 1
            b.unary(u >> k)
            b.put(k, u)


def write_frame(channels, bps, number, block_size=None, assignment="independent", subs=None, rate=44100, variable=False, bps_code=None,
                explicit_block=False):
    """One frame. ``channels``: the samples per channel (stereo undone — what a decoder returns); ``subs``: per coded channel the
    keyword arguments of ``write_subframe`` (default VERBATIM). ``block_size``: the stream's (a shorter frame is coded explicitly)."""
    n = len(channels[0])
    nch = len(channels)
    coded, widths = [list(map(int, c)) for c in channels], [bps] * nch
    ca = ASSIGNMENTS[assignment]
    if ca is not None:
        left, right = coded
        side = [l - r for l, r in zip(left, right)]
        if ca == 8:
            coded, widths = [left, side], [bps, bps + 1]
        elif ca == 9:
            coded, widths = [side, right], [bps + 1, bps]
        else:
            coded, widths = [[(l + r) >> 1 for l, r in zip(left, right)], side], [bps, bps + 1]
    bc = _BLOCK_CODES.get(n) if not explicit_block else None
    if bc is None:
        bc = 6 if n <= 256 else 7
    rc = _RATE_CODES.get(rate, 0)
    head = bytes([0xFF, 0xF8 | (1 if variable else 0), (bc << 4) | rc,
                  ((nch - 1 if ca is None else ca) << 4) | ((_BPS_CODES[bps] if bps_code is None else bps_code) << 1)])
    head += utf8_number(number)
    if bc == 6:
        head += bytes([n - 1])
    elif bc == 7:
        head += (n - 1).to_bytes(2, "big")
    head += bytes([ref.crc8(head)])
    b = Bits()
    for c in range(nch):
        write_subframe(b, coded[c], widths[c], **((subs[c] if subs else None) or {}))
    data = head + b.bytes()
    return data + ref.crc16(data).to_bytes(2, "big")


def write_stream(channels, bps, block_size, first_number=0, assignment="independent", subs=None, rate=44100, **kw):
    """Consecutive frames of ``block_size`` samples (the remainder as a shorter last frame) with one set of choices for all."""
    total = len(channels[0])
    out, k = [], 0
    for at in range(0, total, block_size):
        out.append(write_frame([c[at:at + block_size] for c in channels], bps, first_number + k, block_size, assignment, subs, rate, **kw))
        k += 1
    return b"".join(out)


def file_bytes(frames, bps, nch, block_size, total, rate=44100, extra_blocks=()):
    """``fLaC``, STREAMINFO, ``extra_blocks`` (``(type, body)`` pairs: PADDING, VORBIS_COMMENT, ...) and the frames."""
    v = (rate << 44) | ((nch - 1) << 41) | ((bps - 1) << 36) | total
    info = block_size.to_bytes(2, "big") * 2 + bytes(6) + v.to_bytes(8, "big") + bytes(16)
    blocks = [(0, info)] + list(extra_blocks)
    out = b"fLaC"
    for i, (kind, body) in enumerate(blocks):
        out += bytes([kind | (0x80 if i == len(blocks) - 1 else 0)]) + len(body).to_bytes(3, "big") + body
    return out + frames


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
def _noise(n, bps, seed, amp=0.25, step=1):
    """A smooth signal with noise on top, inside ``amp`` of full scale, in multiples of ``step``."""
    rng = np.random.RandomState(seed)
    full = (1 << (bps - 1)) - 1
    t = np.arange(n)
    x = amp * full * (0.6 * np.sin(t * 0.013 * (1 + seed % 5)) + 0.4 * rng.uniform(-1, 1, n))
    return [int(v) // step * step for v in x]


def _lpc(order, precision, shift, seed, negative=True):
    """Small coefficients that keep the residual inside 32 bits for any input: sum |c| <= 2^shift (so the prediction is no larger
    than the largest sample)."""
    rng = np.random.RandomState(seed)
    cap = max(1, min((1 << shift) // order, (1 << (precision - 1)) - 1))
    c = [int(v) for v in rng.randint(-cap if negative else 0, cap + 1, order)]
    if negative and all(v >= 0 for v in c):
        c[0] = -cap
    return c


def corpus():
    """``[(name, stream bytes, channels as lists, bps, block size)]``: the smallest shapes at which a decoder can go wrong."""
    out = []

    def add(name, chans, bps, bs, **kw):
        out.append((name, write_stream(chans, bps, bs, **kw), [list(c) for c in chans], bps, bs))

    # block sizes (with a final short frame of 1 and of 17 samples), partition order 0 and the largest that divides the block
    # (the short last frame takes neither the order nor the partitions: it is FIXED 0 in one partition)
    for bs, tail, po in ((16, 1, 4), (192, 17, 6), (4096, 1, 12), (4608, 17, 9), (16384, 0, 14)):
        n = 2 * bs + tail
        x = _noise(n, 16, bs)
        rest = write_stream([x[2 * bs:]], 16, bs, first_number=2, subs=[dict(kind="FIXED", order=0, porder=0, params=[12])]) if tail else b""
        whole = write_stream([x[:2 * bs]], 16, bs, subs=[dict(kind="FIXED", order=2, porder=0, params=[9])])
        out.append((f"fixed2_bs{bs}_p0", whole + rest, [x], 16, bs))
        # the largest partition order that divides the block: partitions of bs >> po samples, the first one shorter by the order (at a
        # partition of one sample: empty)
        order = min(2, bs >> po)
        whole = write_stream([x[:2 * bs]], 16, bs, subs=[dict(kind="FIXED", order=order, porder=po, params=[9] * (1 << po))])
        out.append((f"fixed{order}_bs{bs}_p{po}", whole + rest, [x], 16, bs))
    # a first partition exactly as long as the predictor order: no residual in it
    x = _noise(64, 16, 3)
    add("fixed4_first_partition_empty", [x], 16, 64, subs=[dict(kind="FIXED", order=4, porder=4, params=[8] * 16)])
    # Rice parameters 0, 14 and 30; escapes of 0 and of 17 raw bits; a unary run of more than 64 zero bits
    add("rice0_long_unary", [[0] * 8 + [40, -40] + [0] * 6], 16, 16, subs=[dict(kind="FIXED", order=0, porder=0, params=[0])])
    x = _noise(32, 16, 5)
    add("rice14", [x], 16, 16, subs=[dict(kind="FIXED", order=0, porder=0, params=[14], method=0)])
    add("rice30", [_noise(32, 24, 6)], 24, 16, subs=[dict(kind="FIXED", order=0, porder=0, params=[30], method=1)])
    add("escape0", [[7] * 4 + [7] * 28], 16, 32, subs=[dict(kind="FIXED", order=1, porder=1, params=[("escape", 0), ("escape", 0)])])
    add("escape17", [_noise(32, 16, 7)], 16, 32, subs=[dict(kind="FIXED", order=0, porder=1, params=[("escape", 17), 11])])
    # FIXED orders 0..4
    for o in range(5):
        add(f"fixed{o}", [_noise(80, 16, 10 + o)], 16, 32, subs=[dict(kind="FIXED", order=o, porder=1, params=[10, 11])])
    # LPC orders 1, 8, 12, 32; precision 15 with shift 0 and 14; negative coefficients
    for o, prec, sh in ((1, 15, 0), (8, 15, 14), (12, 12, 9), (32, 15, 14), (8, 5, 3)):
        add(f"lpc{o}_q{prec}_s{sh}", [_noise(192, 16, 20 + o)], 16, 64,
            subs=[dict(kind="LPC", coefs=_lpc(o, prec, sh, o), precision=prec, shift=sh, porder=1, params=[12, 13])])
    # full-magnitude 15-bit coefficients (+16383, -16384, ...) at shift 0 and 14 on a small signal: the sign extension at full precision,
    # products of 2^14 x 2^9 summed over 8 terms in 64 bits (|samples| < 2^9 keeps the shift-0 residual under 2^27)
    small = [int(v) for v in 400 * np.sin(np.arange(192) * 0.07) + np.random.RandomState(77).randint(-60, 61, 192)]
    full = [16383, -16384, 16383, -16384, 16000, -16383, 16384 - 1, -16384]
    for sh in (0, 14):
        add(f"lpc8_full_q15_s{sh}", [small], 16, 64, subs=[dict(kind="LPC", coefs=full, precision=15, shift=sh, porder=1, params=[22 if sh == 0 else 9, ("escape", 29 if sh == 0 else 14)])])
    # wasted bits 1 and 7
    add("wasted1_fixed", [_noise(64, 16, 30, step=2)], 16, 32, subs=[dict(kind="FIXED", order=2, porder=0, params=[9], wasted=1)])
    add("wasted7_lpc", [_noise(64, 24, 31, step=128)], 24, 32,
        subs=[dict(kind="LPC", coefs=_lpc(4, 10, 6, 9), precision=10, shift=6, porder=0, params=[14], wasted=7)])
    add("wasted7_constant_verbatim", [[384] * 32, _noise(32, 16, 32, step=128)], 16, 32,
        subs=[dict(kind="CONSTANT", wasted=7), dict(kind="VERBATIM", wasted=7)])
    # sample sizes
    for bps in (8, 12, 16, 20, 24):
        add(f"bps{bps}", [_noise(50, bps, bps, amp=0.9), _noise(50, bps, bps + 1, amp=0.9)], bps, 32,
            subs=[dict(kind="FIXED", order=1, porder=0, params=[max(bps - 4, 1)], method=1), dict(kind="VERBATIM")])
    # channels 1, 2, 8; the four assignments; full-scale antiphase stereo at 24 bits: a 25-bit side channel
    add("ch8", [_noise(40, 16, 40 + c) for c in range(8)], 16, 16, subs=[dict(kind="FIXED", order=c % 5, porder=0, params=[11]) for c in range(8)])
    l, r = _noise(70, 16, 50), _noise(70, 16, 51)
    for a in ("independent", "left_side", "side_right", "mid_side"):
        add(f"stereo_{a}", [l, r], 16, 32, assignment=a, subs=[dict(kind="FIXED", order=1, porder=0, params=[11], method=1)] * 2)
    top = (1 << 23) - 1
    anti_l, anti_r = [top, -top - 1] * 16, [-top - 1, top] * 16
    for a in ("left_side", "side_right", "mid_side"):
        add(f"antiphase24_{a}", [anti_l, anti_r], 24, 32, assignment=a, subs=[dict(kind="VERBATIM")] * 2)
    # frame numbers 127/128 and 2047/2048 at block size 16
    for first in (127, 2047):
        add(f"number{first}", [_noise(48, 16, first)], 16, 16, first_number=first, subs=[dict(kind="FIXED", order=1, porder=0, params=[10])])
    return out
