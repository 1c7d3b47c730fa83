// JS value coercion for the units that read SceneData (scene.cpp, scene_gen.cpp): ToNumber,
// truthiness, String() and the Vec3 spread for the JSON-representable values we accept. Inline,
// host only, so that neither unit depends on the other.
#pragma once

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "json.hpp"
#include "rt_math.hpp"

namespace rt {

using rtj::Value;

constexpr double kPI = 3.141592653589793;  // Math.PI

[[noreturn]] inline void fail(const std::string& msg) { throw std::runtime_error(msg); }

// ToNumber for the JSON-representable JS values we accept.
inline double to_number(const Value* v, double dflt) {
    if (!v) return dflt;  // property absent -> default parameter / undefined handling by caller
    switch (v->kind) {
        case Value::Number: return v->num;
        case Value::Bool: return v->b ? 1.0 : 0.0;
        case Value::Null: return 0.0;
        case Value::String: {
            const char* s = v->str.c_str();
            char* e = nullptr;
            double d = std::strtod(s, &e);
            while (e && (*e == ' ' || *e == '\t' || *e == '\n')) ++e;
            if (v->str.empty()) return 0.0;
            return (e && *e == '\0') ? d : NAN;
        }
        default: return NAN;
    }
}

inline bool truthy(const Value* v) {
    if (!v) return false;
    switch (v->kind) {
        case Value::Null: return false;
        case Value::Bool: return v->b;
        case Value::Number: return !(v->num == 0.0 || std::isnan(v->num));
        case Value::String: return !v->str.empty();
        default: return true;
    }
}

inline std::string js_string(const Value* v) {
    if (!v) return "undefined";
    switch (v->kind) {
        case Value::Null: return "null";
        case Value::Bool: return v->b ? "true" : "false";
        case Value::String: return v->str;
        case Value::Number: { std::string s; rtj::dump_number(s, v->num); return s; }
        case Value::Object: return "[object Object]";
        case Value::Array: {
            std::string s;
            for (size_t i = 0; i < v->arr.size(); ++i) { if (i) s += ","; s += js_string(&v->arr[i]); }
            return s;
        }
    }
    return "";
}

// Vec3.create(...array): spread of a 3-array into Float32Array stores
// (missing entries are undefined -> NaN). Non-iterables throw a TypeError.
inline V3 vec_from(const Value* v, const char* what) {
    if (!v || !v->is_array()) fail(std::string(what) + " is not iterable");
    double c[3] = {NAN, NAN, NAN};
    for (size_t i = 0; i < 3 && i < v->arr.size(); ++i) c[i] = to_number(&v->arr[i], NAN);
    return mk<double>(c[0], c[1], c[2]);
}

inline std::string num_str(double v) { std::string s; rtj::dump_number(s, v); return s; }

}  // namespace rt
