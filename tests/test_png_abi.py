"""The device PNG encoder (png_deflate.hpp), run on the host by rt_debug_png_host, block by block
(CPU). Every frame of the case table (tests/png_cases.py) and of test_abi.py's _png_frames is
encoded once; the row filters and the filtered stream are compared with their restatement
(tests/png_ref.py), the deflate blocks are read by png_ref.inspect - itself compared with zlib -
and each case's witness must hold. Every comparison is exact."""
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_cases  # noqa: E402
import png_ref  # noqa: E402
from test_abi import _png_frames  # noqa: E402

EXISTING = dict(_png_frames())
_ENCODED = {}


def encoded(rt, name):
    """{label: (png, Enc)} of a case, or of one of the older frames; encoded once."""
    from raytracer_amd.png import debug_png_host
    if name not in _ENCODED:
        frames = png_cases.frames(name) if name in png_cases.CASES else {name: EXISTING[name]}
        done = {}
        for label, f in frames.items():
            png = debug_png_host(f.tobytes(), f.shape[1], f.shape[0])
            done[label] = (png, png_cases.read(f, png))
        _ENCODED[name] = done
    return _ENCODED[name]


ALL = list(png_cases.CASES) + list(EXISTING)


def test_reader_agrees_with_zlib_on_zlib_streams():
    """png_ref.inspect on streams zlib itself wrote - stored, fixed and dynamic blocks, real
    distances, a sync flush in the middle: it decodes what zlib decodes, and refuses damage."""
    rng = np.random.default_rng(1)
    text = bytes(rng.choice(np.frombuffer(b"abcdefgh \n", np.uint8), 5000, p=[.3, .2, .1, .1, .1, .05, .05, .04, .05, .01]))
    datas = [b"", b"a", bytes(300), text, rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), text[:700] * 5]
    kinds = set()
    for data in datas:
        for level in (0, 1, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY):
                c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
                z = c.compress(data[:len(data) // 2]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[len(data) // 2:])
                z += c.flush()
                blocks = png_ref.inspect(z)
                assert png_ref.inflate(blocks) == zlib.decompress(z) == data
                assert sum(b["zbytes"] for b in blocks) <= len(z) - 6 + len(blocks)
                assert sum(b["raw"] for b in blocks) == len(data) and blocks[-1]["final"]
                kinds |= {b["btype"] for b in blocks}
                for b in blocks:
                    if b["btype"] == 2:
                        assert len(b["ll_lengths"]) == b["hlit"] and len(b["dist_lengths"]) == b["hdist"]
                        assert png_ref.kraft(b["ll_lengths"]) == 1 and png_ref.kraft(b["cl_lengths"]) == 1
    assert kinds == {0, 1, 2}
    z = bytearray(zlib.compress(text, 6))
    z[-1] ^= 1
    with pytest.raises(ValueError):
        png_ref.inspect(z)                # the Adler-32
    with pytest.raises(ValueError):
        png_ref.inspect(z[:len(z) // 2])  # cut off


def test_min_depth_restatement():
    """min_depth against trees small enough to see: a chain, a balanced tree, a tie that a deeper
    merge order would lose, and the Lucas histogram of the ll-limit case."""
    assert png_ref.min_depth([]) == 0 and png_ref.min_depth([0, 5, 0]) == 1 and png_ref.min_depth([1, 9]) == 1
    assert png_ref.min_depth([1] * 8) == 3 and png_ref.min_depth([1] * 9) == 4
    assert png_ref.min_depth([1, 1, 2, 4, 8, 16]) == 5          # powers of two: a chain
    assert png_ref.min_depth([1, 1, 2, 2]) == 2                 # leaves first on ties: 2, not 3
    assert png_ref.min_depth(png_cases.LUCAS_COUNTS) == 15
    assert png_ref.min_depth(png_cases.LUCAS_COUNTS + [1]) == 16


@pytest.mark.parametrize("name", ALL)
def test_png_decodes_to_the_frame(rt, name):
    from raytracer_amd.png import decode_png_rgb
    for label, (png, enc) in encoded(rt, name).items():
        h, w, _ = enc.frame.shape
        assert decode_png_rgb(png) == (w, h, enc.frame.tobytes()), label


@pytest.mark.parametrize("name", ALL)
def test_filters_and_stream_equal_the_restatement(rt, name):
    """Row by row the filter type is the min-sum choice (ties to the lower type, 0x80 counts 128),
    and the stream zlib decompresses is the restated filtered stream."""
    for label, (png, enc) in encoded(rt, name).items():
        h, w, _ = enc.frame.shape
        raw = zlib.decompress(png_ref.zlib_stream(png))
        want = png_ref.choose_filters(enc.frame)
        got = np.frombuffer(raw, np.uint8)[::3 * w + 1]
        assert len(raw) == h * (3 * w + 1) and np.array_equal(got, want), (label, np.flatnonzero(got != want)[:8])
        assert raw == png_ref.filtered_stream(enc.frame, want), label


@pytest.mark.parametrize("name", ALL)
def test_blocks(rt, name):
    """The container and the block structure: zlib header 78 01 in a single IDAT; the reader
    agrees with zlib; one block per 4096 stream bytes, each of the right raw size; every block
    but the last is non-final and ends on a sync flush unless it is stored; the last is final;
    every dynamic block's three codes are complete and its tokens are the greedy distance-1 /
    distance-3 runs DESIGN.md describes, with RFC 1951's length symbols (258 is symbol 285)."""
    for label, (png, enc) in encoded(rt, name).items():
        z = png_ref.zlib_stream(png)                    # asserts the single IDAT
        assert z[:2] == b"\x78\x01", label
        assert enc.stream == zlib.decompress(z), label
        h, w, _ = enc.frame.shape
        total = h * (3 * w + 1)
        n = -(-total // png_ref.SEG)
        assert [b["raw"] for b in enc.blocks] == [png_ref.SEG] * (n - 1) + [total - png_ref.SEG * (n - 1)], label
        assert sum(b["zbytes"] for b in enc.blocks) == len(z) - 6, label       # byte-aligned, nothing between
        want = png_ref.run_tokens(enc.stream)
        for k, b in enumerate(enc.blocks):
            assert bool(b["final"]) == (k == n - 1), (label, k)
            assert b["btype"] in (0, 2) and b["flush"] == (b["btype"] == 2 and k < n - 1), (label, k)
            if b["btype"] == 0:
                assert b["zbytes"] == b["raw"] + 5, (label, k)
                continue
            assert b["zbytes"] < b["raw"] + 5, (label, k)                       # else it would be stored
            for code in ("ll_lengths", "dist_lengths", "cl_lengths"):
                assert png_ref.kraft(b[code]) == 1, (label, k, code)
            assert max(b["ll_lengths"] + b["dist_lengths"]) <= 15 and max(b["cl_lengths"]) <= 7, (label, k)
            assert [t[:2] if isinstance(t, tuple) else t for t in b["tokens"]] == want[k], (label, k)
            for t in b["tokens"]:
                assert not isinstance(t, tuple) or t[2] == png_ref.length_symbol(t[0]), (label, k, t)


@pytest.mark.parametrize("name", list(png_cases.CASES))
def test_witness(rt, name):
    """The case reaches the path it is named for (tests/png_cases.py)."""
    png_cases.CASES[name][1]({label: enc for label, (_, enc) in encoded(rt, name).items()})


def test_the_limiters_are_rare_elsewhere(rt):
    """What makes ll-limit and cl-limit needed: in every other frame here no literal/length code
    wants more than 15 bits, so without ll-limit no test would see that limiter work."""
    deep = set()
    for name in ALL:
        for label, (_, enc) in encoded(rt, name).items():
            if any(b["btype"] == 2 and png_ref.min_depth(png_cases.ll_hist(b)) > 15 for b in enc.blocks):
                deep.add(name)
    assert deep == {"ll-limit"}
