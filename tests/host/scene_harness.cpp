// Stand-alone harness of the host units that take untrusted bytes: json.hpp, scene.cpp,
// scene_tree.cpp, scene_gen.cpp, scene_blob.cpp and prog_blob.cpp. tests/test_host_sanitizers.py
// compiles it with AddressSanitizer and UBSan and runs it as a child process; a caught exception
// is a fine outcome of any input, a sanitizer report ends the run.
//
//   scene_harness <cases.json> <checkpoint.bin> [dom mutations per scene] [text mutations per scene] [blob mutations]
//
// cases.json: [{"name", "scene", "options"}, ...], the table of tests/degenerate_cases.py, the
// base scene first. (a) every case builds a scene and its blob; (b) mutations of the parsed DOM
// of the default scene and of the base scene, each dumped, parsed again and built; (c) mutations
// of their text; (d) the checkpoint with header fields changed and both checksums made to fit,
// and with its end cut off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "json.hpp"
#include "prog_blob.hpp"
#include "scene.hpp"
#include "scene_blob.hpp"

using rtj::Value;

namespace {

struct Rng {  // splitmix64: the harness must not depend on the library's generator
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

std::string read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

struct Tally {
    long built = 0, refused = 0;
};

// parse -> build_scene -> build_scene_blob; true when all three went through
bool build_text(const std::string& scene, const std::string* options, Tally& t) {
    try {
        const Value sd = rtj::parse(scene);
        Value ro;
        if (options) ro = rtj::parse(*options);
        const rt::SceneBuild b = rt::build_scene(sd, options ? &ro : nullptr);
        const rt::SceneBlob blob = rt::build_scene_blob(b);
        (void)blob;
        (void)rt::prog_fingerprint(b);
        ++t.built;
        return true;
    } catch (const std::exception&) {
        ++t.refused;
        return false;
    }
}

// ---- (b) mutations of the DOM -----------------------------------------------------------------
void collect(Value& v, std::vector<Value*>& all) {
    all.push_back(&v);
    for (Value& x : v.arr) collect(x, all);
    for (rtj::Member& m : v.obj) collect(m.second, all);
}

const double kNumbers[] = {NAN, INFINITY, -INFINITY, 0.0, -0.0, 1e308, 1e-320, 1e39, -1.0, 2.5};

void mutate_dom(Value& root, Rng& r) {
    std::vector<Value*> all;
    collect(root, all);
    std::vector<Value*> numbers, objects, strings;
    for (Value* v : all) {
        if (v->is_number()) numbers.push_back(v);
        if (v->is_object() && !v->obj.empty()) objects.push_back(v);
        if (v->is_string()) strings.push_back(v);
    }
    switch (r.below(6)) {
        case 0:  // a number becomes a hostile one
            if (!numbers.empty()) numbers[r.below(numbers.size())]->num = kNumbers[r.below(sizeof kNumbers / sizeof *kNumbers)];
            break;
        case 1: {  // a key disappears
            if (objects.empty()) break;
            Value* o = objects[r.below(objects.size())];
            o->obj.erase(o->obj.begin() + (long)r.below(o->obj.size()));
            break;
        }
        case 2: {  // a value changes its kind
            Value* v = all[r.below(all.size())];
            switch (r.below(6)) {
                case 0: *v = Value::null(); break;
                case 1: *v = Value::boolean(r.below(2) != 0); break;
                case 2: *v = Value::number(kNumbers[r.below(sizeof kNumbers / sizeof *kNumbers)]); break;
                case 3: *v = Value::string(r.below(2) ? "" : "lambert"); break;
                case 4: *v = Value::array(); break;
                default: *v = Value::object(); break;
            }
            break;
        }
        case 3: {  // a string (a material id, a type) becomes another string of the scene
            if (strings.size() < 2) break;
            const std::string other = strings[r.below(strings.size())]->str;
            strings[r.below(strings.size())]->str = other;
            break;
        }
        default: {  // an entry of objects / materials is doubled or dropped
            Value* list = const_cast<Value*>(root.get(r.below(2) ? "objects" : "materials"));
            if (!list || !list->is_array() || list->arr.empty()) break;
            const size_t k = r.below(list->arr.size());
            if (r.below(2)) {
                const Value copy = list->arr[k];
                list->arr.push_back(copy);
            } else {
                list->arr.erase(list->arr.begin() + (long)k);
            }
            break;
        }
    }
}

void dom_mutations(const Value& scene, const std::string& options, long n, uint64_t seed, Tally& t) {
    Rng r{seed};
    for (long i = 0; i < n; ++i) {
        Value v = scene;
        for (size_t k = 1 + r.below(3); k > 0; --k) mutate_dom(v, r);
        build_text(rtj::dump(v), &options, t);
    }
}

// ---- (c) mutations of the text -----------------------------------------------------------------
void text_mutations(const std::string& text, const std::string& options, long n, uint64_t seed, Tally& t) {
    static const char* kTokens[] = {"NaN", "Infinity", "-Infinity", "null", "true", "[", "]", "{", "}", ",", ":", "\"",
                                    "1e999", "-0", "\\u", "\\", "0x1", ".", "e", "-"};
    Rng r{seed};
    for (long i = 0; i < n; ++i) {
        std::string s = text;
        for (size_t k = 1 + r.below(3); k > 0 && !s.empty(); --k) {
            const size_t at = r.below(s.size());
            switch (r.below(5)) {
                case 0: s[at] = (char)r.below(256); break;
                case 1: s.erase(at, 1 + r.below(8)); break;
                case 2: s.insert(at, kTokens[r.below(sizeof kTokens / sizeof *kTokens)]); break;
                case 3: s.insert(at, s.substr(r.below(s.size()), r.below(40))); break;
                default: s.resize(at); break;
            }
        }
        // the options text takes a share of the mutations too
        if (i % 8 == 7) build_text(text, &s, t);
        else build_text(s, &options, t);
    }
}

// ---- (d) the checkpoint ------------------------------------------------------------------------
void seal(std::vector<uint8_t>& blob) {  // make both checksums fit what the blob now holds
    rt::ProgBlobHeader h;
    std::memcpy(&h, blob.data(), sizeof h);
    const size_t payload = blob.size() - sizeof h;
    h.payload_checksum = rt::fnv1a(blob.data() + sizeof h, (size_t)std::min<uint64_t>(h.payload_bytes, payload));
    h.header_checksum = rt::fnv1a(&h, offsetof(rt::ProgBlobHeader, header_checksum));
    std::memcpy(blob.data(), &h, sizeof h);
}

bool parse_blob(const std::vector<uint8_t>& blob, size_t len, Tally& t) {
    try {
        const rt::ProgBlobHeader h = rt::prog_parse_blob(blob.data(), len);
        rt_progressive_info info;
        rt::prog_info_from_header(h, &info);
        ++t.built;
        return true;
    } catch (const std::exception&) {
        ++t.refused;
        return false;
    }
}

void blob_mutations(const std::string& file, long n, uint64_t seed, Tally& t) {
    const std::vector<uint8_t> good(file.begin(), file.end());
    if (!parse_blob(good, good.size(), t)) throw std::runtime_error("the checkpoint fixture does not parse");
    static const int64_t kInts[] = {0, 1, -1, 7, 8, 9, 63, 64, 65, 0x7fffffff, -0x7fffffff - 1, 0x7ffffff8, 0x7ffffff9,
                                    0x40000000, 1 << 20, 65535, 65536};
    Rng r{seed};
    for (long i = 0; i < n; ++i) {
        std::vector<uint8_t> blob = good;
        rt::ProgBlobHeader h;
        std::memcpy(&h, blob.data(), sizeof h);
        for (size_t k = 1 + r.below(3); k > 0; --k) {
            const int32_t v = (int32_t)kInts[r.below(sizeof kInts / sizeof *kInts)];
            switch (r.below(14)) {
                case 0: h.width = v; break;
                case 1: h.height = v; break;
                case 2: h.rx = v; break;
                case 3: h.ry = v; break;
                case 4: h.rw = v; break;
                case 5: h.rh = v; break;
                case 6: h.precision = v; break;
                case 7: h.samples_loop = v; break;
                case 8: h.samples_done = v; break;
                case 9: h.steps = v; break;
                case 10: h.active_pixels = r.below(2) ? (int64_t)v : (int64_t)r.next(); break;
                case 11: h.payload_bytes = r.below(2) ? (uint64_t)(int64_t)v : r.next(); break;
                case 12: h.samples = kNumbers[r.below(sizeof kNumbers / sizeof *kNumbers)]; break;
                default: {  // a small region whose payload fits inside the fixture's
                    h.rw = 1 + (int32_t)r.below(16);
                    h.rh = 1 + (int32_t)r.below(16);
                    h.payload_bytes = (uint64_t)((h.rw + 7) / 8) * (uint64_t)((h.rh + 7) / 8) * 64 * rt::kProgPixBytes;
                    blob.resize(sizeof h + (size_t)h.payload_bytes);
                    break;
                }
            }
        }
        std::memcpy(blob.data(), &h, sizeof h);
        seal(blob);
        parse_blob(blob, blob.size(), t);
        // cut off: inside the header, inside the payload, one byte short
        const size_t cuts[] = {r.below(sizeof h), sizeof h + r.below(blob.size() - sizeof h + 1), blob.size() - 1};
        parse_blob(blob, cuts[r.below(3)], t);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: scene_harness cases.json checkpoint.bin [dom] [text] [blob]\n");
        return 2;
    }
    const long n_dom = argc > 3 ? std::atol(argv[3]) : 2000;
    const long n_text = argc > 4 ? std::atol(argv[4]) : 20000;
    const long n_blob = argc > 5 ? std::atol(argv[5]) : 2000;
    try {
        // (a) every case of the table
        const Value cases = rtj::parse(read_file(argv[1]));
        if (!cases.is_array() || cases.arr.empty()) throw std::runtime_error("cases.json: not a list of cases");
        Tally ta;
        for (const Value& c : cases.arr) {
            const Value* name = c.get("name");
            const Value* scene = c.get("scene");
            const Value* options = c.get("options");
            if (!name || !scene || !options) throw std::runtime_error("cases.json: a case needs name, scene and options");
            const std::string ro = rtj::dump(*options);
            if (!build_text(rtj::dump(*scene), &ro, ta)) {
                std::fprintf(stderr, "case %s does not build\n", name->str.c_str());
                return 1;
            }
        }
        std::printf("cases: %ld built\n", ta.built);

        const Value& base = *cases.arr[0].get("scene");
        const std::string base_ro = rtj::dump(*cases.arr[0].get("options"));
        const Value dflt = rt::generate_scene_data("default", nullptr);

        Tally tb, tc, td;
        dom_mutations(dflt, base_ro, n_dom, 1, tb);
        dom_mutations(base, base_ro, n_dom, 2, tb);
        std::printf("dom mutations: %ld built, %ld refused\n", tb.built, tb.refused);
        text_mutations(rtj::dump(dflt), base_ro, n_text, 3, tc);
        text_mutations(rtj::dump(base), base_ro, n_text, 4, tc);
        std::printf("text mutations: %ld built, %ld refused\n", tc.built, tc.refused);
        blob_mutations(read_file(argv[2]), n_blob, 5, td);
        std::printf("checkpoint mutations: %ld parsed, %ld refused\n", td.built, td.refused);
        if (tb.built == 0 || tb.refused == 0 || tc.built == 0 || tc.refused == 0 || td.built < 2 || td.refused == 0) {
            std::fprintf(stderr, "a mutation family never built or never failed: it tests nothing\n");
            return 1;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "harness: %s\n", e.what());
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
