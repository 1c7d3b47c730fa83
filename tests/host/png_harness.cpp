// Stand-alone harness of the device PNG encoder's per-segment routine, rtpng::deflate_segment
// (png_deflate.hpp), on the host. tests/test_host_sanitizers.py compiles it with AddressSanitizer
// and UBSan, links zlib and runs it as a child process; a sanitizer report or a mismatch ends the
// run.
//
//   png_harness [random segments] [seed]
//
// Every segment is encoded twice over differently poisoned scratch (the bytes must not depend on
// what an earlier segment left behind), inflated with raw zlib - inflateSetDictionary with the
// bytes of `hist` that exist - and compared: the bytes, the Adler-32 of the raw bytes, the CRC-32
// of the compressed bytes, len <= kOutCap, and the place where the block ends (a non-final block
// must leave zlib on a byte boundary between blocks). Segments: random alphabets (uniform,
// geometric, Zipf) and run densities, lengths 1...4096, q0 of 0...3 and beyond, hist that does
// and does not continue a run (for q0 < 4 the bytes before the stream are filled with what a run
// would want to see), final and non-final; the Lucas histogram that needs the 15-bit limiter; the
// 1x1 black frame, whose tokens are read from the tokeniser's array.
// Prints how many segments were stored and how many needed each limiter.
#include <zlib.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "png_deflate.hpp"

using rtpng::SegResult;
using rtpng::SegWork;

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return n ? (uint32_t)(next() % n) : 0; }
    double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
};

[[noreturn]] void fail(const char* what, long seg) {
    std::printf("FAILED: %s (segment %ld)\n", what, seg);
    std::exit(1);
}

// Depth of a minimum-depth Huffman tree over the non-zero counts: two queues, a leaf before an
// internal node of the same weight.
int min_depth(const uint32_t* freq, int n) {
    std::vector<uint64_t> leaf;
    for (int i = 0; i < n; ++i)
        if (freq[i]) leaf.push_back(freq[i]);
    if (leaf.size() < 2) return (int)leaf.size();
    for (size_t i = 1; i < leaf.size(); ++i)  // insertion sort
        for (size_t j = i; j > 0 && leaf[j - 1] > leaf[j]; --j) std::swap(leaf[j - 1], leaf[j]);
    std::vector<uint64_t> w;
    std::vector<int> h;
    size_t i = 0, j = 0;
    auto take = [&](uint64_t& weight, int& height) {
        if (i < leaf.size() && (j >= w.size() || leaf[i] <= w[j])) {
            weight = leaf[i++];
            height = 0;
        } else {
            weight = w[j];
            height = h[j++];
        }
    };
    for (size_t k = 0; k + 1 < leaf.size(); ++k) {
        uint64_t w1, w2;
        int h1, h2;
        take(w1, h1);
        take(w2, h2);
        w.push_back(w1 + w2);
        h.push_back((h1 > h2 ? h1 : h2) + 1);
    }
    return h.back();
}

struct Tally {
    long segments = 0, stored = 0, ll_limited = 0, cl_limited = 0;
};

struct Harness {
    std::unique_ptr<SegWork> W{new SegWork};
    uint32_t table[256];
    Tally t;

    Harness() {
        for (uint32_t i = 0; i < 256; ++i) table[i] = rtpng::crc_table_entry(i);
    }

    SegResult encode(const std::vector<uint8_t>& f, const uint8_t hist[4], int64_t q0, bool final, uint8_t poison) {
        std::memset((void*)W.get(), poison, sizeof(SegWork));
        std::memcpy(W->hist, hist, 4);
        std::memcpy(W->f, f.data(), f.size());
        return rtpng::deflate_segment(*W, (int)f.size(), q0, final, table);
    }

    // One segment; returns with W holding the second run's scratch.
    void check(const std::vector<uint8_t>& f, const uint8_t hist[4], int64_t q0, bool final) {
        const long id = t.segments++;
        const int n = (int)f.size();
        const SegResult r0 = encode(f, hist, q0, final, 0x00);
        if (r0.len > (uint32_t)rtpng::kOutCap) fail("len > kOutCap", id);
        const std::vector<uint8_t> first(W->out, W->out + r0.len);
        const SegResult r = encode(f, hist, q0, final, 0xA5);
        if (r.len != r0.len || r.crc != r0.crc || r.adler != r0.adler || r.raw != r0.raw ||
            std::memcmp(first.data(), W->out, r.len) != 0)
            fail("the bytes depend on stale scratch", id);
        if (r.raw != (uint32_t)n) fail("raw", id);
        if (r.adler != (uint32_t)adler32(adler32(0L, Z_NULL, 0), f.data(), (uInt)n)) fail("Adler-32", id);
        if (r.crc != (uint32_t)crc32(crc32(0L, Z_NULL, 0), W->out, (uInt)r.len)) fail("CRC-32", id);
        const int btype = (W->out[0] >> 1) & 3;
        if ((W->out[0] & 1) != (final ? 1 : 0) || (btype != 0 && btype != 2)) fail("block header", id);
        if (btype == 0 && r.len != (uint32_t)n + 5) fail("stored size", id);
        if (btype == 2 && r.len >= (uint32_t)n + 5) fail("a dynamic block no smaller than a stored one", id);

        // raw inflate; a non-final segment gets an empty final stored block behind it
        std::vector<uint8_t> in(W->out, W->out + r.len);
        if (!final) {
            const uint8_t end[5] = {1, 0, 0, 0xff, 0xff};
            in.insert(in.end(), end, end + 5);
        }
        std::vector<uint8_t> out((size_t)n + 16);
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) fail("inflateInit2", id);
        const int valid = q0 < 4 ? (int)q0 : 4;
        if (valid > 0 && inflateSetDictionary(&zs, hist + 4 - valid, (uInt)valid) != Z_OK)
            fail("inflateSetDictionary", id);
        zs.next_in = in.data();
        zs.avail_in = (uInt)in.size();
        zs.next_out = out.data();
        zs.avail_out = (uInt)out.size();
        const int rc = inflate(&zs, Z_FINISH);
        const bool good = rc == Z_STREAM_END && zs.avail_in == 0 && zs.total_out == (uLong)n &&
                          std::memcmp(out.data(), f.data(), (size_t)n) == 0;
        inflateEnd(&zs);
        if (!good) fail("zlib does not inflate the segment to its bytes", id);

        // the histograms the encoder left in its scratch: was a limiter needed?
        if (btype == 0) {
            ++t.stored;
        } else {
            const bool ll = min_depth(W->freq, rtpng::kLL) > rtpng::kMaxLL;
            const bool cl = min_depth(W->freq + rtpng::kLL + rtpng::kDist, rtpng::kCL) > rtpng::kMaxCL;
            int max_ll = 0, max_cl = 0;
            for (int s = 0; s < rtpng::kLL + rtpng::kDist; ++s) max_ll = W->len[s] > max_ll ? W->len[s] : max_ll;
            for (int s = 0; s < rtpng::kCL; ++s) {
                const int l = W->len[rtpng::kLL + rtpng::kDist + s];
                max_cl = l > max_cl ? l : max_cl;
            }
            if (max_ll > rtpng::kMaxLL || max_cl > rtpng::kMaxCL) fail("a code longer than its limit", id);
            if (ll && max_ll != rtpng::kMaxLL) fail("15-bit limiter", id);
            if (cl && max_cl != rtpng::kMaxCL) fail("7-bit limiter", id);
            t.ll_limited += ll;
            t.cl_limited += cl;
        }
    }
};

// n bytes: an alphabet of k values under one of three distributions, with runs at distance 1 and
// 3 started with probability `runs`.
std::vector<uint8_t> random_segment(Rng& g, int n) {
    static const int sizes[] = {1, 2, 3, 5, 16, 64, 256};
    const int k = sizes[g.below(7)];
    const int dist = (int)g.below(3);
    const double runs = (g.below(4) == 0) ? 0.0 : g.unit() * g.unit() * 0.3;
    uint8_t alphabet[256];
    for (int i = 0; i < 256; ++i) alphabet[i] = (uint8_t)i;
    for (int i = 255; i > 0; --i) std::swap(alphabet[i], alphabet[g.below((uint32_t)i + 1)]);
    std::vector<double> cum((size_t)k);
    double total = 0;
    for (int i = 0; i < k; ++i) {
        double p = 1;
        if (dist == 1) p = std::exp(-0.25 * i);
        if (dist == 2) p = std::exp(-1.44 * std::log(1.0 + i));
        cum[(size_t)i] = total += p;
    }
    std::vector<uint8_t> f((size_t)n);
    for (int i = 0; i < n;) {
        if (i >= 3 && g.unit() < runs) {
            const int d = g.below(2) ? 1 : 3;
            int len = 1 + (int)g.below(g.below(8) == 0 ? 700 : 12);
            for (; len > 0 && i < n; --len, ++i) f[(size_t)i] = f[(size_t)(i - d)];
            continue;
        }
        const double u = g.unit() * total;
        int s = 0;
        while (s + 1 < k && cum[(size_t)s] < u) ++s;
        f[(size_t)i++] = alphabet[s];
    }
    return f;
}

// The bytes of the Lucas histogram (png_cases.py's ll-limit) in an order with nothing to match.
std::vector<uint8_t> lucas_segment(Rng& g) {
    static const int value[16] = {0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8};
    static const int count[16] = {1366, 843, 521, 322, 199, 123, 76, 47, 29, 18, 11, 7, 4, 3, 1, 1};
    for (;;) {
        int left[16];
        int total = 0;
        for (int i = 0; i < 16; ++i) total += left[i] = count[i];
        std::vector<uint8_t> f;
        while (total > 0) {
            int ok[16], sum = 0;
            const size_t m = f.size();
            for (int i = 0; i < 16; ++i) {
                const uint8_t v = (uint8_t)value[i];
                const bool run1 = m >= 3 && f[m - 1] == v && f[m - 2] == v && f[m - 3] == v;
                const bool run3 = m >= 5 && f[m - 3] == v && f[m - 1] == f[m - 4] && f[m - 2] == f[m - 5];
                sum += ok[i] = (run1 || run3) ? 0 : left[i];
            }
            if (!sum) break;
            int pick = (int)g.below((uint32_t)sum), i = 0;
            while (pick >= ok[i]) pick -= ok[i++];
            f.push_back((uint8_t)value[i]);
            --left[i];
            --total;
        }
        if (!total) return f;
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 3000;
    Rng g{argc > 2 ? (uint64_t)std::atoll(argv[2]) : 20240607ull};
    Harness H;
    static const int64_t q0s[] = {0, 1, 2, 3, 4, 5, 4096, 8192, (int64_t)1 << 20, ((int64_t)1 << 33) + 4096};
    static const int edge_n[] = {1, 2, 3, 4, 5, 257, 258, 259, 260, 4095, 4096};

    for (long k = 0; k < n_random; ++k) {
        int n;
        const uint32_t pick = g.below(10);
        if (pick == 0) n = edge_n[g.below(11)];
        else if (pick < 4) n = 1 + (int)g.below(64);
        else n = 1 + (int)g.below(4096);
        const std::vector<uint8_t> f = random_segment(g, n);
        const int64_t q0 = q0s[g.below(10)];
        uint8_t hist[4];
        for (int i = 0; i < 4; ++i) hist[i] = (uint8_t)g.next();
        if (g.below(2)) {  // continue a run: what distance 1 and distance 3 would look back at
            hist[3] = f[0];
            hist[1] = f[0];
            if (n > 1) hist[2] = f[1];
            if (g.below(2) && n > 2) hist[3] = f[2];
        }
        H.check(f, hist, q0, g.below(2) != 0);
    }

    // the 15-bit limiter: the Lucas histogram, alone in the stream and behind other segments
    for (int k = 0; k < 6; ++k) {
        const std::vector<uint8_t> f = lucas_segment(g);
        const uint8_t hist[4] = {9, 9, 9, 9};  // no byte of the histogram: the tokens are the literals
        const long before = H.t.ll_limited;
        H.check(f, hist, k < 2 ? 0 : 4096 * k, (k & 1) != 0);
        if (H.t.ll_limited != before + 1) fail("the Lucas histogram did not need the 15-bit limiter", H.t.segments - 1);
    }

    // the 1x1 black frame: stored, but tokenised as the literal 0 and a match of 3 at distance 1
    {
        const std::vector<uint8_t> f(4, 0);
        const uint8_t hist[4] = {0, 0, 0, 0};
        H.check(f, hist, 0, true);
        if (H.W->tok[0] != 0u || H.W->tok[1] != (0x80000000u | 3u)) fail("1x1 black: tokens", H.t.segments - 1);
        if (((H.W->out[0] >> 1) & 3) != 0) fail("1x1 black: not stored", H.t.segments - 1);
    }

    std::printf("segments: %ld, stored: %ld, ll-limited: %ld, cl-limited: %ld\nok\n", H.t.segments, H.t.stored,
                H.t.ll_limited, H.t.cl_limited);
    return 0;
}
