"""The STREAMINFO MD5 of FLAC delivery without a GPU (option "flac_md5"; elementary_amd/csrc/flac_md5.h).

1. FlacMd5 — elemhip_flac_md5_init / _update / _final, which walk the kernel's schedule of chunks serially — against hashlib.md5 over
   the same codes packed by numpy: every padding residue, messages under one block, the empty message.
2. Updates in pieces, and the record's size.
3. The option on a dry handle.
4. The container: a file written with patch(md5=...) verifies — its announced MD5 is that of its own decoded samples.

The oracle is exact, so nothing here has a tolerance."""
import hashlib

import numpy as np
import pytest

import flac_reference as ref

EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")


def _codes(G, n, bits, seed=1):
    rng = np.random.default_rng(seed * 1000003 + 97 * G + bits + 7 * n)
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(G, n), dtype=np.int64).astype(np.int32)
    if n >= 2:
        x[0, 0], x[-1, -1] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1          # both ends of the range
    return x


def packed(codes, bits):
    """int [G, n] -> the interleaved little-endian bytes process_blocks_pcm delivers in s16 / s24."""
    a = np.ascontiguousarray(np.asarray(codes, dtype=np.int32).T)
    if bits == 16:
        return a.astype("<i2").tobytes()
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(a.shape[0], a.shape[1], 4)[:, :, :3]).tobytes()


def _digest(codes, bits):
    from elementary_amd.runtime import FlacMd5
    return FlacMd5().update(codes, bits).digest()


# ---- 1. against hashlib ------------------------------------------------------------------------------------------------------------------
# mono s24: 64, 43, 61, 40, 21 frames leave 0, 1, 55, 56, 63 bytes behind the last whole block; mono s16: 32 and 28 leave 0 and 56
RESIDUES = {24: ((64, 0), (43, 1), (61, 55), (40, 56), (21, 63)), 16: ((32, 0), (28, 56))}


@pytest.mark.parametrize("bits", [16, 24])
def test_every_padding_residue_mono(bits):
    for n, residue in RESIDUES[bits]:
        assert (n * bits // 8) % 64 == residue
        x = _codes(1, n, bits)
        assert _digest(x, bits) == hashlib.md5(packed(x, bits)).digest(), (bits, n)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_random_codes_equal_hashlib(G, bits):
    """Frame counts whose byte totals leave 0, 1, 55, 56 and 63 bytes (where G and the sample size can), and ones that cross a chunk of
    64 blocks and two."""
    B = bits // 8
    want = {0, 1, 55, 56, 63}
    counts = []
    for n in range(1, 400):
        r = (n * G * B) % 64
        if r in want:
            want.discard(r)
            counts.append(n)
    counts += [4096 // (G * B) + 3, 2 * 4096 // (G * B) + 11, 4 * 256 + 37]
    for n in counts:
        x = _codes(G, n, bits)
        assert _digest(x, bits) == hashlib.md5(packed(x, bits)).digest(), (G, bits, n)


def test_under_one_block_and_the_empty_message():
    from elementary_amd.runtime import FlacMd5
    x = _codes(1, 5, 16)
    assert len(packed(x, 16)) == 10 and _digest(x, 16) == hashlib.md5(packed(x, 16)).digest()
    assert FlacMd5().digest() == EMPTY == hashlib.md5(b"").digest()
    assert FlacMd5().update(np.zeros((2, 0), dtype=np.int32), 24).digest() == EMPTY


# ---- 2. pieces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,bits", [(1, 16), (2, 24), (3, 24), (8, 16)])
def test_pieces_give_the_one_piece_digest(G, bits):
    from elementary_amd.runtime import FlacMd5, load_library
    n = 5 * 256 + 101
    x = _codes(G, n, bits, seed=2)
    h = FlacMd5()
    assert h.record.nbytes == int(load_library().elemhip_flac_md5_record_bytes()) and h.record.nbytes % 16 == 0
    at = 0
    for m in (1, 37, 350, n):
        m = min(m, n - at)
        h.update(x[:, at:at + m], bits)
        at += m
        assert h.digest() == hashlib.md5(packed(x[:, :at], bits)).digest()        # (a digest in between leaves the record as it was)
    assert at == n and h.digest() == _digest(x, bits)


def test_refused_arguments():
    from elementary_amd.runtime import ElemHipError, FlacMd5
    for codes, bits in ((np.zeros((9, 4), dtype=np.int32), 16), (np.zeros((1, 4), dtype=np.int32), 20)):
        with pytest.raises(ElemHipError):
            FlacMd5().update(codes, bits)


# ---- 3. the option on a dry handle -------------------------------------------------------------------------------------------------------
def test_option_values_on_a_dry_handle():
    from elementary_amd.runtime import ElemHipError, Runtime
    dry = Runtime(44100.0, 64, device=-1)
    for good in (1, 0, 1.0):
        dry.set_option("flac_md5", good)
    for bad in (2, 0.5, -1):
        with pytest.raises(ElemHipError) as e:
            dry.set_option("flac_md5", bad)
        assert e.value.code == 6
    got = dry.flac_read()
    assert got["md5_state"] == 0 and got["md5"] == []


# ---- 4. the container --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,bits", [(1, 16), (2, 24)])
def test_a_patched_file_verifies(tmp_path, G, bits):
    from elementary_amd.flac import FlacReader, FlacWriter, streaminfo
    from elementary_amd.runtime import FlacMd5, flac_encode
    n = 256 * 4 + 31
    x = _codes(G, n, bits, seed=3)
    data, lens = flac_encode(x, bits=bits, flac_frame=256, sample_rate=48000)
    digest = FlacMd5().update(x, bits).digest()
    for name, md5 in (("with.flac", digest), ("without.flac", None)):
        path = tmp_path / name
        w = FlacWriter(path, bits, G, 48000, 256)
        w.write(data)
        w.patch(len(lens), int(lens.min()), int(lens.max()), n, **({} if md5 is None else {"md5": md5}))
        w.close()
        info, _, chans = ref.decode_file(path.read_bytes())
        own = hashlib.md5(packed(np.array(chans, dtype=np.int64), bits)).digest()
        assert info["total"] == n and (info["min_frame"], info["max_frame"]) == (int(lens.min()), int(lens.max()))
        if md5 is None:
            assert info["md5"] == bytes(16) and FlacReader(str(path)).md5 == bytes(16)
        else:
            assert info["md5"] == own and info["md5"] != bytes(16)         # the file verifies
            assert FlacReader(str(path)).md5 == own
    assert streaminfo(256, bits, G, 48000, md5=digest)[18:] == digest and streaminfo(256, bits, G, 48000)[18:] == bytes(16)
    with pytest.raises(ValueError):
        streaminfo(256, bits, G, 48000, md5=b"short")
