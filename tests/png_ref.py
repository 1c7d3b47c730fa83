"""Independent restatements for the device PNG encoder's tests (NumPy / pure Python, no project
code): the PNG row filters and the min-sum filter choice (RFC 2083 §6), a bit-level deflate
reader that reports what an encoder emitted (RFC 1950 / 1951), the depth of a minimum-depth
Huffman tree, and the encoder's documented token rule (greedy runs at distance 1 and 3).

Nothing here is shared with png_deflate.hpp; the reader is itself pinned to zlib by
tests/test_png_abi.py (its output must equal zlib.decompress of the same stream)."""
from fractions import Fraction

import numpy as np

SEG = 4096      # filtered-stream bytes per deflate block of the device encoder
MAX_RUN = 258


# ---------------------------------------------------------------- PNG filters (RFC 2083 §6)

def residuals(rgb):
    """(H, 5, 3W) uint8: every row filtered with each of the five types. The first row sees a row
    of zeros above it, the first pixel sees zeros to its left."""
    rgb = np.asarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    raw = rgb.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, 3:] = raw[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth], axis=1)
    return (out & 255).astype(np.uint8)


def filter_sums(rgb):
    """(H, 5) int64: the sum over a row of |residual|, the residuals read as signed bytes (0x80
    counts 128)."""
    r = residuals(rgb).astype(np.int64)
    return np.where(r >= 128, 256 - r, r).sum(axis=2)


def choose_filters(rgb):
    """(H,) uint8: per row the filter type with the least sum; ties go to the lower type."""
    return np.argmin(filter_sums(rgb), axis=1).astype(np.uint8)   # argmin: the first minimum


def filtered_stream(rgb, ftypes):
    """The filtered scanline stream: per row the filter type byte, then the 3W filtered bytes."""
    r = residuals(rgb)
    h = r.shape[0]
    ftypes = np.asarray(ftypes, np.uint8)
    rows = r[np.arange(h), ftypes]
    return np.concatenate([ftypes[:, None], rows], axis=1).tobytes()


# ---------------------------------------------------------------- deflate reader (RFC 1951)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos = data, pos * 8     # pos: a bit index

    def get(self, n):
        v = 0
        for i in range(n):
            if self.pos >> 3 >= len(self.d):
                raise ValueError("deflate stream ends inside a block")
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


def kraft(lengths):
    """The Kraft sum of a code's lengths (zero = unused), exactly."""
    return sum((Fraction(1, 1 << int(n)) for n in lengths if n), Fraction(0))


def _table(lengths):
    """(length, code) -> symbol of the canonical code (RFC 1951 §3.2.2)."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    table = {}
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def _sym(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.get(1)      # Huffman codes are packed most significant bit first
        s = table.get((n, code))
        if s is not None:
            return s
    raise ValueError("bit pattern that is no code word")


def inspect(zlib_bytes):
    """Reads a zlib stream block by block. Returns a list of dicts:
      final, btype, raw (bytes the block decodes to), data (those bytes), zbytes (compressed bytes
      the block occupies: up to the next byte boundary, an immediately following empty non-final
      stored block - a sync flush - included), flush (whether that empty block followed),
      tokens (a literal as an int, a match as (length, distance, length symbol); none for btype 0),
    and for btype 2: hlit, hdist, hclen (the counts, not the header fields), cl_lengths (19, by
    symbol), ll_lengths (hlit), dist_lengths (hdist), cl_stream (a list of (symbol, extra value)).
    Checks the zlib header and the Adler-32 trailer; raises ValueError on a malformed stream."""
    d = bytes(zlib_bytes)
    if len(d) < 6 or (d[0] & 15) != 8 or ((d[0] << 8) | d[1]) % 31 or d[1] & 0x20:
        raise ValueError("not a zlib stream without a preset dictionary")
    bits = _Bits(d, 2)
    out = bytearray()
    blocks = []
    fixed_ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    while True:
        start = bits.pos
        blk = {"final": bits.get(1), "btype": bits.get(2), "tokens": [], "flush": False}
        at = len(out)
        if blk["btype"] == 0:
            bits.align()
            n, nn = bits.get(16), bits.get(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("stored block: LEN and NLEN disagree")
            p = bits.pos >> 3
            if p + n > len(d):
                raise ValueError("stored block runs past the stream")
            if blocks and n == 0 and not blk["final"] and blocks[-1]["btype"] != 0 and not blocks[-1]["flush"] \
                    and blocks[-1]["end"] == start:
                blocks[-1]["flush"] = True      # the sync flush belongs to the block it follows
                blocks[-1]["end"] = bits.pos
                continue
            out += d[p:p + n]
            bits.pos += 8 * n
        elif blk["btype"] in (1, 2):
            if blk["btype"] == 1:
                ll, dl = fixed_ll, [5] * 30
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits.get(3)
                clt = _table(cl)
                lens, stream = [], []
                while len(lens) < hlit + hdist:
                    s = _sym(bits, clt)
                    if s < 16:
                        stream.append((s, 0))
                        lens.append(s)
                        continue
                    ev = bits.get({16: 2, 17: 3, 18: 7}[s])
                    stream.append((s, ev))
                    if s == 16:
                        if not lens:
                            raise ValueError("repeat code with nothing to repeat")
                        lens += [lens[-1]] * (3 + ev)
                    else:
                        lens += [0] * ((3 if s == 17 else 11) + ev)
                if len(lens) != hlit + hdist:
                    raise ValueError("code lengths overrun HLIT + HDIST")
                ll, dl = lens[:hlit], lens[hlit:]
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=cl, ll_lengths=ll, dist_lengths=dl,
                           cl_stream=stream)
            llt, dt = _table(ll), _table(dl)
            while True:
                s = _sym(bits, llt)
                if s < 256:
                    out.append(s)
                    blk["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol past 285")
                    length = LEN_BASE[s - 257] + bits.get(LEN_EXTRA[s - 257])
                    ds = _sym(bits, dt)
                    if ds > 29:
                        raise ValueError("distance symbol past 29")
                    dist = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise ValueError("distance reaches before the stream")
                    for _ in range(length):
                        out.append(out[-dist])
                    blk["tokens"].append((length, dist, s))
        else:
            raise ValueError("block type 3")
        blk["start"], blk["end"] = start, bits.pos
        blk["data"] = bytes(out[at:])
        blk["raw"] = len(out) - at
        blocks.append(blk)
        if blk["final"]:
            break
    bits.align()
    p = bits.pos >> 3
    if len(d) != p + 4:
        raise ValueError("bytes after the final block and its Adler-32")
    a, b = 1, 0
    for v in out:
        a = (a + v) % 65521
        b = (b + a) % 65521
    if int.from_bytes(d[p:], "big") != (b << 16 | a):
        raise ValueError("Adler-32 does not match")
    for blk in blocks:
        blk["zbytes"] = ((blk["end"] + 7) >> 3) - (blk["start"] >> 3)
    return blocks


def inflate(blocks):
    """The bytes inspect() decoded."""
    return b"".join(b["data"] for b in blocks)


def zlib_stream(png):
    """The zlib stream of a PNG file that has exactly one IDAT chunk."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, []
    while pos < len(png):
        n = int.from_bytes(png[pos:pos + 4], "big")
        if png[pos + 4:pos + 8] == b"IDAT":
            idat.append(png[pos + 8:pos + 8 + n])
        pos += 12 + n
    assert pos == len(png) and len(idat) == 1
    return idat[0]


# ---------------------------------------------------------------- Huffman depth

def min_depth(freqs):
    """Depth of a minimum-depth Huffman tree over the non-zero frequencies: the two-queue merge
    in which a leaf is taken before an internal node of the same weight. A code-length limiter is
    needed exactly when this exceeds the limit. One used symbol: 1 (deflate spends a bit on it)."""
    leaves = sorted(int(f) for f in freqs if f)
    if len(leaves) < 2:
        return len(leaves)
    nodes = []                 # (weight, height) of internal nodes, in order of creation
    i = j = 0

    def take():
        nonlocal i, j
        if i < len(leaves) and (j >= len(nodes) or leaves[i] <= nodes[j][0]):
            i += 1
            return leaves[i - 1], 0
        j += 1
        return nodes[j - 1]

    for _ in range(len(leaves) - 1):
        (w1, h1), (w2, h2) = take(), take()
        nodes.append((w1 + w2, max(h1, h2) + 1))
    return nodes[-1][1]


# ---------------------------------------------------------------- the encoder's token rule

def run_tokens(stream, seg=SEG):
    """Per segment of `seg` stream bytes, the tokens DESIGN.md §4 describes: greedy; at each
    position the run at distance 1 (the previous byte) and at distance 3 (the previous pixel's
    channel), each at most 258 and ending with the segment; the longer one, distance 1 on a tie,
    is a match if it is at least 3 long, else the byte is a literal. A match may start at a
    segment's first byte and reach into the segment before it, never before the stream (no
    distance-1 match at stream position 0, no distance-3 match before position 3). The distance-3
    run is not looked at once the distance-1 run has reached 258. Matches are
    (length, distance), literals ints."""
    s = bytes(stream)
    out = []
    for q0 in range(0, len(s), seg):
        end = min(len(s), q0 + seg)
        toks = []
        q = q0
        while q < end:
            best = {}
            for d in (1, 3):
                n = 0
                if q >= d:
                    while q + n < end and n < MAX_RUN and s[q + n] == s[q + n - d]:
                        n += 1
                best[d] = n
            if best[1] == MAX_RUN:
                best[3] = 0
            n, d = (best[1], 1) if best[1] >= best[3] else (best[3], 3)
            if n >= 3:
                toks.append((n, d))
                q += n
            else:
                toks.append(s[q])
                q += 1
        out.append(toks)
    return out


def length_symbol(length):
    """The literal/length symbol of a match length (RFC 1951 §3.2.5): 258 is 285, not 284."""
    if length == 258:
        return 285
    return 257 + max(k for k in range(28) if LEN_BASE[k] <= length)
