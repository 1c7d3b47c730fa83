"""The device PNG encoder's case table: small frames, one per path of png_deflate.hpp, each with
a witness. A witness is a property read out of the emitted bit stream by png_ref.inspect (an
independent deflate reader) that proves the frame went down the path it was written for, so a
case cannot silently stop covering it when the encoder or the frame changes.

CASES maps a name to (build, witness). build() returns {label: (H, W, 3) uint8 frame}, always
the same frames (fixed numpy Generator seeds; searched seeds and recipes are written out here).
witness(encs) takes {label: Enc} - the frame, its decompressed filtered stream and the blocks
png_ref.inspect read from its zlib stream - and asserts. No project code is used here."""
from collections import namedtuple

import numpy as np

import png_ref

Enc = namedtuple("Enc", "frame stream blocks")   # (H, W, 3) uint8, bytes, list of inspect() blocks

SEG = png_ref.SEG


# ---------------------------------------------------------------- helpers

def frame_of_stream(stream, w):
    """The one-row frame whose filtered stream under filter 0 is `stream` (stream[0] == 0)."""
    assert stream[0] == 0 and len(stream) == 3 * w + 1
    return np.array(stream[1:], np.uint8).reshape(1, w, 3)


def _forbidden(out, v):
    """Would appending v complete a run a match could take: four equal bytes, or six with period 3?"""
    if len(out) >= 3 and out[-1] == v and out[-2] == v and out[-3] == v:
        return True
    return len(out) >= 5 and out[-3] == v and out[-1] == out[-4] and out[-2] == out[-5]


def place(counts, seed, head=(0,)):
    """The bytes of `counts` ({value: count}, `head` included) in a weighted random order that
    leaves the tokeniser nothing to match; None when the draw paints itself into a corner."""
    rng = np.random.default_rng(seed)
    left = dict(counts)
    out = list(head)
    for v in head:
        left[v] -= 1
    for _ in range(sum(left.values())):
        vals = [v for v, c in left.items() if c > 0 and not _forbidden(out, v)]
        if not vals:
            return None
        pick = int(rng.integers(sum(left[v] for v in vals)))     # one of the bytes still to place
        for v in vals:
            pick -= left[v]
            if pick < 0:
                break
        out.append(v)
        left[v] -= 1
    return out


def positions(blk_tokens, start):
    """(stream position, token) of a block's tokens; the block starts at `start`."""
    p = start
    for t in blk_tokens:
        yield p, t
        p += t[0] if isinstance(t, tuple) else 1


def ll_hist(blk):
    """The literal/length histogram a dynamic block's tokens give, the end-of-block included."""
    h = [0] * 286
    for t in blk["tokens"]:
        h[t[2] if isinstance(t, tuple) else t] += 1
    h[256] += 1
    return h


def cl_hist(blk):
    h = [0] * 19
    for s, _ in blk["cl_stream"]:
        h[s] += 1
    return h


def matches(enc):
    return [t for b in enc.blocks for t in b["tokens"] if isinstance(t, tuple)]


def ftypes_of(enc):
    h, w, _ = enc.frame.shape
    return [enc.stream[y * (3 * w + 1)] for y in range(h)]


def only(encs):
    (enc,) = encs.values()
    return enc


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter_row(t, resid, prev):
    """The raw row whose residual under filter t, below the raw row `prev`, is `resid`."""
    cur = [0] * len(resid)
    for x in range(len(resid)):
        a = cur[x - 3] if x >= 3 else 0
        b = int(prev[x])
        c = int(prev[x - 3]) if x >= 3 else 0
        pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]
        cur[x] = (int(resid[x]) + pred) & 255
    return cur


# ---------------------------------------------------------------- the limiters

LUCAS_VALUES = [0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8]
LUCAS_COUNTS = [1366, 843, 521, 322, 199, 123, 76, 47, 29, 18, 11, 7, 4, 3, 1, 1]
LL_LIMIT_SEED = 0     # the first seed at which place() finishes


def build_ll_limit():
    """1190x1. With the end-of-block the histogram is 1, 1, 1, 3, 4, 7, 11, ... (Lucas numbers):
    each merge joins the subtree built so far with the next leaf, so the tree is a chain 16 deep -
    the deepest a segment's tokens can give, one past the 15 bits deflate allows."""
    s = place(dict(zip(LUCAS_VALUES, LUCAS_COUNTS)), LL_LIMIT_SEED)
    assert s is not None
    return {"lucas": frame_of_stream(s, 1190)}


def witness_ll_limit(encs):
    enc = only(encs)
    assert ftypes_of(enc) == [0]
    (blk,) = enc.blocks
    assert blk["btype"] == 2 and not matches(enc)
    assert png_ref.min_depth(ll_hist(blk)) == 16
    assert max(blk["ll_lengths"]) == 15
    assert png_ref.kraft(blk["ll_lengths"]) == 1


CL_LIMIT_SEED = 5     # searched on the host run of the encoder: seeds 5, 9, 17 and 19 of 0...24 do it


def build_cl_limit():
    """100x1, Zipf-distributed bytes (p_k ~ k^-1.44) over a shuffled alphabet. Such a source has
    about 1.618^L symbols of probability 2^-L, so the literal code's lengths occur 1, 1, 2, 3, 5,
    8, ... times: a Fibonacci histogram of code-length symbols, which plain Huffman codes more
    than 7 deep once nine lengths are in use."""
    rng = np.random.default_rng(CL_LIMIT_SEED)
    pr = 1 / np.arange(1, 257) ** 1.44
    return {"zipf": rng.permutation(256)[rng.choice(256, (1, 100, 3), p=pr / pr.sum())].astype(np.uint8)}


def witness_cl_limit(encs):
    (blk,) = only(encs).blocks
    assert blk["btype"] == 2
    assert png_ref.min_depth(cl_hist(blk)) > 7
    assert max(blk["cl_lengths"]) == 7
    assert png_ref.kraft(blk["cl_lengths"]) == 1


# ---------------------------------------------------------------- length codes

def _runs_stream():
    """One row of zero runs under filter 0. A run of N is N + 1 zeros after a non-zero separator
    byte: the first zero is a literal (it equals neither its left neighbour nor, for more than
    two bytes, the bytes three back), the other N are distance-1 matches. No run crosses a
    segment boundary: separators pad the segment's end instead. Returns (stream, {N: position of
    the run's first zero})."""
    lengths = list(range(3, 259)) + [259, 260, 261, 516]
    s, where, sep = [0], {}, 0

    def separator():
        nonlocal sep
        sep += 1                      # 1, 2, -1, -2 in turn: no two equal within three bytes, and
        s.append((1, 2, 255, 254)[sep % 4])     # Sub gains nothing on a stretch of them

    separator()
    for n in lengths:
        while (len(s) + 1) // SEG != (len(s) + n + 2) // SEG:    # separator + run would cross
            separator()
        separator()
        where[n] = len(s)
        s.extend([0] * (n + 1))
    separator()
    while len(s) % 3 != 1:
        separator()
    return s, where


def build_length_codes():
    """Nine segments: runs of every length 3...258 alone are 33 KB of stream."""
    s, _ = _runs_stream()
    return {"runs": frame_of_stream(s, (len(s) - 1) // 3)}


def witness_length_codes(encs):
    enc = only(encs)
    assert ftypes_of(enc) == [0]
    _, where = _runs_stream()
    toks = {}
    for k, blk in enumerate(enc.blocks):
        assert blk["btype"] == 2
        toks.update(positions(blk["tokens"], k * SEG))
    assert {t[2] for t in matches(enc)} == set(range(257, 286))      # every length symbol
    for n in range(3, 259):
        assert toks[where[n]] == 0 and toks[where[n] + 1] == (n, 1, png_ref.length_symbol(n)), n
    assert toks[where[258] + 1] == (258, 1, 285)                      # not 284 + 31 extra
    assert [toks.get(where[259] + 1 + i) for i in (0, 258)] == [(258, 1, 285), 0]
    assert [toks.get(where[260] + 1 + i) for i in (0, 258, 259)] == [(258, 1, 285), 0, 0]
    assert [toks.get(where[261] + 1 + i) for i in (0, 258)] == [(258, 1, 285), (3, 1, 257)]
    assert [toks.get(where[516] + 1 + i) for i in (0, 258)] == [(258, 1, 285), (258, 1, 285)]


# ---------------------------------------------------------------- distances

def _ramp(w):
    """One row whose Sub residual is the same pixel (3, 7, 250) everywhere: the filtered stream
    has period 3 and no byte equals its neighbour. (A frame of one constant pixel cannot give a
    distance-3 match: Sub and Up turn it into zeros, which are distance-1 runs.)"""
    x = np.arange(1, w + 1)
    return np.stack([x * 3, x * 7, x * 250], -1).astype(np.uint8).reshape(1, w, 3)


def _dist_witness(enc, dist, hdist, dist_lengths):
    assert {t[1] for t in matches(enc)} == {dist}
    for blk in enc.blocks:
        assert blk["btype"] == 2
        if any(isinstance(t, tuple) for t in blk["tokens"]):
            # an unused distance code 0 / 1 is sent with one dummy count, so that the code is complete
            assert (blk["hdist"], blk["dist_lengths"]) == (hdist, dist_lengths)


def _run_lengths(s, q, end):
    out = {}
    for d in (1, 3):
        n = 0
        while q >= d and q + n < end and n < 258 and s[q + n] == s[q + n - d]:
            n += 1
        out[d] = n
    return out


def build_d1_only():
    return {"flat": np.full((3, 20, 3), 77, np.uint8)}


def witness_d1_only(encs):
    enc = only(encs)
    _dist_witness(enc, 1, 2, [1, 1])
    (blk,) = enc.blocks
    for p, t in positions(blk["tokens"], 0):       # and nowhere was there a choice to make
        if isinstance(t, tuple):
            assert _run_lengths(enc.stream, p, len(enc.stream))[3] < 3


def build_d3_only():
    return {"ramp": _ramp(200)}


def witness_d3_only(encs):
    enc = only(encs)
    assert ftypes_of(enc) == [1]
    _dist_witness(enc, 3, 3, [2, 2, 1])


def build_d1_d3_tie():
    return {"black": np.zeros((2, 120, 3), np.uint8)}


def witness_d1_d3_tie(encs):
    enc = only(encs)
    _dist_witness(enc, 1, 2, [1, 1])
    (blk,) = enc.blocks
    ties = 0
    for p, t in positions(blk["tokens"], 0):
        if isinstance(t, tuple):
            r = _run_lengths(enc.stream, p, len(enc.stream))
            ties += 3 <= r[1] == r[3] < 258
    assert ties >= 1


def build_boundary_d1():
    return {"flat": np.full((6, 300, 3), 17, np.uint8)}        # 5406 stream bytes


def build_boundary_d3():
    return {"ramp": _ramp(2000)}                               # 6001 stream bytes


def _boundary_witness(enc, dist):
    assert len(enc.blocks) >= 2
    for blk in enc.blocks[1:]:
        t = blk["tokens"][0]
        assert isinstance(t, tuple) and t[1] == dist     # position 0 of its segment: reaches back
    assert {t[1] for t in matches(enc)} == {dist}


def witness_boundary_d1(encs):
    _boundary_witness(only(encs), 1)


def witness_boundary_d3(encs):
    _boundary_witness(only(encs), 3)


# ---------------------------------------------------------------- the start of the stream

def build_stream_start():
    """The four smallest frames, and two whose blocks are long enough to be dynamic. (A stream of
    4 to 8 bytes always costs less stored - 5 bytes of header against 14 or more of code tables -
    so the tokens of the four are not in their bit streams; tests/host/png_harness.cpp reads the
    1x1 black frame's "literal 0, match (3, 1)" out of the tokeniser's own array.)"""
    rng = np.random.default_rng(11)
    x = np.arange(1, 41)
    return {"1x1-black": np.zeros((1, 1, 3), np.uint8),
            "1x1-random": rng.integers(1, 256, (1, 1, 3), dtype=np.uint8),
            "1x2": np.zeros((2, 1, 3), np.uint8),
            "2x1": np.array([[[2, 0, 1], [4, 0, 2]]], np.uint8),
            # all zeros: position 0 equals the zero "before the stream", and must be a literal
            "20x1-black": np.zeros((1, 20, 3), np.uint8),
            # Sub residuals (2, 0, 1) everywhere behind the filter byte 1: at position 2 the bytes
            # 0, 1, 2, ... equal "three back" if the zeros before the stream counted
            "40x1-period3": np.stack([2 * x, 0 * x, x], -1).astype(np.uint8).reshape(1, 40, 3)}


def witness_stream_start(encs):
    for label, enc in encs.items():
        (blk,) = enc.blocks
        assert blk["btype"] == (2 if label in ("20x1-black", "40x1-period3") else 0), label
        for p, t in positions(blk["tokens"], 0):
            assert not isinstance(t, tuple) or p >= t[1], label     # no match reaches before the stream
    assert encs["2x1"].stream == bytes([1, 2, 0, 1, 2, 0, 1])
    assert encs["20x1-black"].blocks[0]["tokens"] == [0, (60, 1, png_ref.length_symbol(60))]
    s = encs["40x1-period3"].stream
    assert s[:3] == bytes([1, 2, 0]) and s[3:] == s[:-3]
    assert encs["40x1-period3"].blocks[0]["tokens"] == [1, 2, 0, (118, 3, png_ref.length_symbol(118))]


# ---------------------------------------------------------------- code-length runs

def _alphabet_frame(symbols, seed):
    """Sixteen byte values, sixteen of each, nothing to match, filter 0: the symbol that sorts
    first and the end-of-block get 5 bits, the others 4, so the used values' spacing is the
    zero runs of the code-length stream and their neighbours its repeats."""
    assert len(symbols) == 16 and symbols[0] == 0
    s = place({v: 16 for v in symbols}, seed)
    assert s is not None
    return frame_of_stream(s, 85)


CL_RUNS_SEEDS = (0, 0)


def build_cl_runs():
    gaps = [0, 3, 7, 18] + list(range(30, 37)) + list(range(175, 179)) + [255]   # zero runs 2, 3, 10, 11, 138
    gap139 = list(range(8)) + list(range(147, 154)) + [255]                        # a zero run of 139
    return {"gaps": _alphabet_frame(gaps, CL_RUNS_SEEDS[0]), "gap139": _alphabet_frame(gap139, CL_RUNS_SEEDS[1])}


def witness_cl_runs(encs):
    seen, zero_runs, eighteen_then_zero = set(), set(), False
    for enc in encs.values():
        assert ftypes_of(enc) == [0]
        (blk,) = enc.blocks
        assert blk["btype"] == 2
        st = blk["cl_stream"]
        seen |= set(st)
        lens = blk["ll_lengths"] + blk["dist_lengths"]
        run = 0
        for v in lens + [1]:
            if v == 0:
                run += 1
            else:
                zero_runs.add(run)
                run = 0
        for i in range(1, len(st) - 2):
            eighteen_then_zero |= (st[i - 1][0] not in (0, 17, 18) and st[i] == (18, 127) and st[i + 1] == (0, 0)
                                   and st[i + 2][0] not in (0, 17, 18))
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= seen
    assert {2, 139} <= zero_runs and eighteen_then_zero


# ---------------------------------------------------------------- stored and dynamic blocks

def build_stored_dynamic_mix():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (20, 100, 3), dtype=np.uint8)
    flat = np.full((20, 100, 3), 90, np.uint8)
    return {"noise-flat": np.concatenate([noise, flat]), "flat-noise": np.concatenate([flat, noise])}


def witness_stored_dynamic_mix(encs):
    pairs, stored = set(), set()
    for enc in encs.values():
        kinds = [b["btype"] for b in enc.blocks]
        pairs |= set(zip(kinds, kinds[1:]))
        stored |= {bool(b["final"]) for b in enc.blocks if b["btype"] == 0}
        for b in enc.blocks:
            assert b["zbytes"] <= b["raw"] + 5 + (0 if b["final"] else 5)
            if b["btype"] == 0:
                assert b["zbytes"] == b["raw"] + 5
    assert {(0, 2), (2, 0)} <= pairs and stored == {False, True}


# ---------------------------------------------------------------- row filters

FILTER_BANDS = (0, 4, 2, 3, 1)     # each band follows rows that make its filter the only good one
FILTERS_SEED = 2
FILTERS_W = 16


def _band_row(t, k, rng, n):
    if t == 0:                                    # rough in every direction
        return rng.integers(-40, 41, n)
    if t == 1:                                    # a smooth walk from a start far from the row above
        r = rng.integers(-2, 3, n)
        r[:3] = (60 if k % 2 else -60) + rng.integers(-5, 6, 3)
        return r
    if t == 4:                                    # follows whichever neighbour Paeth points at
        r = rng.integers(-1, 2, n)
        for x in rng.choice(n // 3, 3, replace=False):
            r[3 * x:3 * x + 3] = rng.integers(40, 100, 3) * rng.choice([-1, 1], 3)
        return r
    return rng.integers(-2, 3, n)                 # Up, Average: close to their prediction


def build_filters():
    """Five bands of five rows; each row is drawn (fixed seed) until the restatement's sum for
    the band's filter is the only least one. Then: a zero row; a smooth row, for which Sub and
    Paeth tie exactly below None and Up (the row above is zero); a zero row; a row of 0x80,
    whose Sub residuals 0x80, 0x80, 0x80, 0, ... win only if 0x80 counts 128."""
    rng = np.random.default_rng(FILTERS_SEED)
    n = 3 * FILTERS_W
    rows = []
    prev = [0] * n
    for t in FILTER_BANDS:
        for k in range(5):
            for _ in range(200):
                raw = unfilter_row(t, _band_row(t, k, rng, n), prev)
                sums = png_ref.filter_sums(np.array([prev, raw], np.uint8).reshape(2, FILTERS_W, 3))[1]
                others = [v for u, v in enumerate(sums) if u != t and (rows or u != 2)]   # row 0: Up is None
                if sums[t] < min(others):
                    break
            else:
                raise AssertionError(f"no row for filter {t}")
            rows.append(raw)
            prev = raw
    walk = unfilter_row(1, _band_row(1, 1, rng, n), [0] * n)
    rows += [[0] * n, walk, [0] * n, [128] * n]
    return {"bands": np.array(rows, np.uint8).reshape(len(rows), FILTERS_W, 3)}


def witness_filters(encs):
    enc = only(encs)
    ft = ftypes_of(enc)
    assert ft[:25] == [t for t in FILTER_BANDS for _ in range(5)] and set(ft) == {0, 1, 2, 3, 4}
    sums = png_ref.filter_sums(enc.frame)
    assert ft[25:] == [0, 1, 0, 1]
    assert sums[26][1] == sums[26][4] < min(sums[26][0], sums[26][2], sums[26][3])     # the tie: the lower type
    assert sums[27][0] == sums[27][1] == 0                                              # and another one
    n = 3 * FILTERS_W
    row = enc.stream[28 * (n + 1):29 * (n + 1)]
    assert row == bytes([1, 128, 128, 128] + [0] * (n - 3))
    r = png_ref.residuals(enc.frame)[28].astype(int)
    for count in (0, -128):                         # 0x80 dropped, or left negative: another choice
        alt = np.where(r == 128, count, np.where(r > 128, 256 - r, r)).sum(axis=1)
        assert int(np.argmin(alt)) != 1


# ---------------------------------------------------------------- geometry

GEOMETRY = {                       # w x h -> the blocks' raw sizes
    (1365, 3): [4096, 4096, 4096],               # a row is exactly one segment
    (1364, 3): [4096, 4096, 4087],               # a row one byte short of a segment
    (1366, 3): [4096, 4096, 4096, 9],            # and one byte past
    (80, 17): [4096, 1],                         # a final segment of one byte
    (1, 1025): [4096, 4],                        # 4-byte rows; a final segment of one row
    (1, 1024): [4096],                           # exactly one full segment
    (1, 257): [1028],                            # more than 256 rows: png_filter_kernel's second group
    (5, 600): [4096, 4096, 1408],
    (4096, 2): [4096] * 6 + [2],                 # a row spanning several segments
}


def _geometry_case(w, h):
    def build():
        rng = np.random.default_rng(1000 * w + h)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx // 7, yy // 3, (xx + yy) // 5], -1)
        return {f"{w}x{h}": ((base + rng.integers(0, 3, (h, w, 3))) % 256).astype(np.uint8)}

    def witness(encs):
        assert [b["raw"] for b in only(encs).blocks] == GEOMETRY[(w, h)]

    return build, witness


CASES = {
    "ll-limit": (build_ll_limit, witness_ll_limit),
    "cl-limit": (build_cl_limit, witness_cl_limit),
    "length-codes": (build_length_codes, witness_length_codes),
    "d1-only": (build_d1_only, witness_d1_only),
    "d3-only": (build_d3_only, witness_d3_only),
    "d1-d3-tie": (build_d1_d3_tie, witness_d1_d3_tie),
    "boundary-d1": (build_boundary_d1, witness_boundary_d1),
    "boundary-d3": (build_boundary_d3, witness_boundary_d3),
    "stream-start": (build_stream_start, witness_stream_start),
    "cl-runs": (build_cl_runs, witness_cl_runs),
    "stored-dynamic-mix": (build_stored_dynamic_mix, witness_stored_dynamic_mix),
    "filters": (build_filters, witness_filters),
}
CASES.update({f"geometry-{w}x{h}": _geometry_case(w, h) for (w, h) in GEOMETRY})

_FRAMES = {}


def read(frame, png):
    """Enc of a frame and the PNG an encoder made of it."""
    z = png_ref.zlib_stream(png)
    blocks = png_ref.inspect(z)
    return Enc(frame, png_ref.inflate(blocks), blocks)


def frames(name):
    """The case's frames, built once."""
    if name not in _FRAMES:
        _FRAMES[name] = CASES[name][0]()
        for f in _FRAMES[name].values():
            f.setflags(write=False)
    return _FRAMES[name]
