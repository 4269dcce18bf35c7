"""A pure-Python FLAC decoder written from RFC 9639, the reference of the FLAC delivery tests.

It decodes what the encoder may produce and nothing it may not hide behind: every frame's CRC-8 and CRC-16 are verified, reserved
values, non-zero padding, trailing or missing bits are errors, and `decode_file` checks the STREAMINFO fields against the frames.
Subframes: CONSTANT, VERBATIM, FIXED 0..4 and LPC (for completeness), partitioned Rice residuals with 4- and 5-bit parameters and
escaped partitions, wasted bits, all four channel assignments."""
import struct


class FlacError(ValueError):
    pass


def crc8(data, crc=0):
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def crc16(data, crc=0):
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


_CRC16_TABLE = [crc16(bytes([i])) for i in range(256)]


def _crc16_fast(data):
    crc = 0
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16_TABLE[(crc >> 8) ^ b]
    return crc


class BitReader:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos * 8

    def read(self, n):
        if n == 0:
            return 0
        end = self.pos + n
        if end > len(self.data) * 8:
            raise FlacError("missing bits")
        lo, hi = self.pos >> 3, (end + 7) >> 3
        v = int.from_bytes(self.data[lo:hi], "big")
        v >>= hi * 8 - end
        self.pos = end
        return v & ((1 << n) - 1)

    def read_signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while True:
            if self.pos >= len(self.data) * 8:
                raise FlacError("missing bits")
            byte, off = self.data[self.pos >> 3], self.pos & 7
            rest = (byte << off) & 0xFF
            if rest == 0:
                q += 8 - off
                self.pos += 8 - off
                continue
            lead = 8 - rest.bit_length()
            self.pos += lead + 1
            return q + lead


_BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_BPS = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def _read_utf8(data, pos):
    b0 = data[pos]
    if b0 < 0x80:
        return b0, pos + 1
    n = 8 - (b0 ^ 0xFF).bit_length()
    if n < 2 or n > 7:
        raise FlacError("bad coded number")
    v = b0 & (0x7F >> n)
    for k in range(1, n):
        b = data[pos + k]
        if b & 0xC0 != 0x80:
            raise FlacError("bad coded number continuation")
        v = (v << 6) | (b & 0x3F)
    return v, pos + n


def _residual(br, n, order, info):
    method = br.read(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits = 4 if method == 0 else 5
    porder = br.read(4)
    if n % (1 << porder) or (n >> porder) < order:
        raise FlacError("partition order does not divide the block")
    info["method"], info["porder"], info["params"] = method, porder, []
    out = []
    for p in range(1 << porder):
        cnt = (n >> porder) - (order if p == 0 else 0)
        k = br.read(pbits)
        if k == (1 << pbits) - 1:
            raw = br.read(5)
            info["params"].append(("escape", raw))
            out.extend(br.read_signed(raw) for _ in range(cnt))
        else:
            info["params"].append(k)
            for _ in range(cnt):
                u = (br.unary() << k) | br.read(k)
                out.append((u >> 1) ^ -(u & 1))
    return out


def _subframe(br, n, bps):
    if br.read(1):
        raise FlacError("subframe padding bit set")
    kind = br.read(6)
    wasted = 0
    if br.read(1):
        wasted = br.unary() + 1
        bps -= wasted
    info = {"wasted": wasted, "bps": bps}
    start = br.pos
    if kind == 0:
        info["kind"] = "CONSTANT"
        s = [br.read_signed(bps)] * n
    elif kind == 1:
        info["kind"] = "VERBATIM"
        s = [br.read_signed(bps) for _ in range(n)]
    elif 8 <= kind <= 12:
        order = kind - 8
        info["kind"], info["order"] = "FIXED", order
        if order > n:
            raise FlacError("predictor order above the block size")
        s = [br.read_signed(bps) for _ in range(order)]
        res = _residual(br, n, order, info)
        c = _FIXED[order]
        for r in res:
            s.append(r + sum(c[j] * s[-1 - j] for j in range(order)))
    elif kind >= 32:
        order = kind - 31
        info["kind"], info["order"] = "LPC", order
        s = [br.read_signed(bps) for _ in range(order)]
        prec = br.read(4) + 1
        if prec == 16:
            raise FlacError("reserved coefficient precision")
        shift = br.read_signed(5)
        if shift < 0:
            raise FlacError("negative predictor shift")
        coef = [br.read_signed(prec) for _ in range(order)]
        for r in _residual(br, n, order, info):
            s.append(r + (sum(coef[j] * s[-1 - j] for j in range(order)) >> shift))
    else:
        raise FlacError("reserved subframe type %d" % kind)
    info["bits"] = br.pos - start + 8
    if wasted:
        s = [v << wasted for v in s]
    return s, info


def decode_frame(data, pos=0, streaminfo=None):
    """One frame at byte `pos`: (frame dict, position behind it). The dict: number, blocksize, rate, bps, assignment, channels (decoded,
    stereo undone), subframes (their kinds and choices), header_bytes, bytes."""
    if len(data) - pos < 6:
        raise FlacError("missing bits")
    if data[pos] != 0xFF or data[pos + 1] & 0xFE != 0xF8:
        raise FlacError("no sync code")
    if data[pos + 1] & 1:
        raise FlacError("variable block size streams are not expected here")
    bc, rc = data[pos + 2] >> 4, data[pos + 2] & 15
    ca, sc = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7
    if data[pos + 3] & 1:
        raise FlacError("reserved header bit set")
    number, p = _read_utf8(data, pos + 4)
    if bc == 0:
        raise FlacError("reserved block size code")
    if bc == 6:
        n = data[p] + 1
        p += 1
    elif bc == 7:
        n = ((data[p] << 8) | data[p + 1]) + 1
        p += 2
    else:
        n = _BLOCK_SIZES[bc]
    if rc == 15:
        raise FlacError("invalid sample rate code")
    if rc == 12:
        rate = data[p] * 1000
        p += 1
    elif rc in (13, 14):
        rate = ((data[p] << 8) | data[p + 1]) * (1 if rc == 13 else 10)
        p += 2
    elif rc == 0:
        rate = streaminfo["rate"] if streaminfo else None
    else:
        rate = _RATES[rc]
    if sc == 3:
        raise FlacError("reserved sample size code")
    bps = streaminfo["bps"] if sc == 0 and streaminfo else _BPS.get(sc)
    if bps is None:
        raise FlacError("sample size unknown")
    if crc8(data[pos:p]) != data[p]:
        raise FlacError("frame header CRC-8 mismatch")
    p += 1
    if ca > 10:
        raise FlacError("reserved channel assignment")
    nch = ca + 1 if ca < 8 else 2
    side = {8: 1, 9: 0, 10: 1}.get(ca)
    br = BitReader(data, p)
    chans, subs = [], []
    for c in range(nch):
        s, info = _subframe(br, n, bps + (1 if side == c else 0))
        chans.append(s)
        subs.append(info)
    pad = -br.pos % 8
    if br.read(pad):
        raise FlacError("non-zero padding")
    end = br.pos >> 3
    if end + 2 > len(data):
        raise FlacError("missing bits")
    if _crc16_fast(data[pos:end]) != (data[end] << 8 | data[end + 1]):
        raise FlacError("frame CRC-16 mismatch")
    if ca == 8:
        chans[1] = [l - s for l, s in zip(chans[0], chans[1])]
    elif ca == 9:
        chans[0] = [s + r for s, r in zip(chans[0], chans[1])]
    elif ca == 10:
        mid, sd = chans
        left = [(((m << 1) | (s & 1)) + s) >> 1 for m, s in zip(mid, sd)]
        chans = [left, [l - s for l, s in zip(left, sd)]]
    lim = 1 << (bps - 1)
    for s in chans:
        if any(v < -lim or v >= lim for v in s):
            raise FlacError("decoded sample out of range")
    frame = {"number": number, "blocksize": n, "rate": rate, "bps": bps, "assignment": ca, "channels": chans, "subframes": subs,
             "header_bytes": p - pos, "bytes": end + 2 - pos}
    return frame, end + 2


def decode_frames(data, streaminfo=None):
    """Every frame of a bare frame sequence; trailing bytes are an error. Returns (frames, channels): the concatenated samples."""
    frames, pos = [], 0
    while pos < len(data):
        f, pos = decode_frame(data, pos, streaminfo)
        if frames and (len(f["channels"]) != len(frames[0]["channels"]) or f["bps"] != frames[0]["bps"]):
            raise FlacError("channel count or sample size changes inside the stream")
        if frames and f["number"] != frames[-1]["number"] + 1:
            raise FlacError("frame numbers are not consecutive")
        frames.append(f)
    chans = [[] for _ in (frames[0]["channels"] if frames else [])]
    for f in frames:
        for c, s in enumerate(f["channels"]):
            chans[c].extend(s)
    return frames, chans


def decode_file(data):
    """A whole .flac file: (streaminfo dict, frames, channels). STREAMINFO is checked against the frames."""
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, info, last = 4, None, False
    while not last:
        if pos + 4 > len(data):
            raise FlacError("missing bits")
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if len(body) != size:
            raise FlacError("missing bits")
        if pos == 4:
            if kind != 0 or size != 34:
                raise FlacError("the first metadata block is not STREAMINFO")
            v = int.from_bytes(body[10:18], "big")
            info = {"min_block": struct.unpack(">H", body[0:2])[0], "max_block": struct.unpack(">H", body[2:4])[0],
                    "min_frame": int.from_bytes(body[4:7], "big"), "max_frame": int.from_bytes(body[7:10], "big"),
                    "rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bps": ((v >> 36) & 31) + 1, "total": v & ((1 << 36) - 1),
                    "md5": bytes(body[18:34])}
        elif kind == 0 or kind == 127:
            raise FlacError("bad metadata block")
        pos += 4 + size
    frames, chans = decode_frames(data[pos:], info)
    total = sum(f["blocksize"] for f in frames)
    if frames:
        if len(chans) != info["channels"] or frames[0]["bps"] != info["bps"]:
            raise FlacError("STREAMINFO channels / sample size do not match the frames")
        if any(f["rate"] != info["rate"] for f in frames):
            raise FlacError("STREAMINFO sample rate does not match the frames")
        if frames[0]["number"] != 0:
            raise FlacError("the first frame is not number 0")
        if any(f["blocksize"] != info["max_block"] for f in frames[:-1]) or frames[-1]["blocksize"] > info["max_block"]:
            raise FlacError("block sizes do not match STREAMINFO")
        if info["min_block"] != info["max_block"]:
            raise FlacError("fixed block size streams carry min = max block size")
        if info["min_frame"] and info["min_frame"] != min(f["bytes"] for f in frames):
            raise FlacError("STREAMINFO minimum frame size is wrong")
        if info["max_frame"] and info["max_frame"] != max(f["bytes"] for f in frames):
            raise FlacError("STREAMINFO maximum frame size is wrong")
    if info["total"] and info["total"] != total:
        raise FlacError("STREAMINFO total samples is wrong")
    return info, frames, chans
