// C ABI of the accumulation across views through specular chains (temporal_spec.hpp): the options,
// the history's chain-guide query and the session and stand-alone accumulate calls - their own
// argument checks in front of api_temporal.cpp's shared bodies (tp_session, tp_explicit). The
// history object, its read-back and its timings are api_temporal.cpp's too.
#include "pass_host.hpp"

using namespace rt;

// rt_specular_temporal_options resolved: a zero field = the default.
struct TsOpts : SpecOpts {
    TpOpts base;
};
static TsOpts ts_resolve(const rt_specular_temporal_options* o, const std::string& who) {
    rt_specular_temporal_options z{};
    if (o) z = *o;
    const TpOpts base = tp_resolve(&z.base, who);  // (its errors first)
    return TsOpts{spec_resolve(z.point_pixels, z.through, who), base};
}

extern "C" {

void rt_specular_temporal_options_default(rt_specular_temporal_options* options) {
    if (options) *options = rt_specular_temporal_options{{0.9f, 0.01f, 0.25f, 256.0f, 0, 2.0f}, 4.0f, 15};
}

int rt_history_chain_guides(const rt_history* h, rt_guide_options* out, int32_t* held) {
    if (!h || !out || !held) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<rt_history*>(h)->mu);
    const rt_history::Side& s = h->side[h->front];
    *held = h->views > 0 && s.has_chain ? 1 : 0;
    *out = *held ? s.chain_go : rt_guide_options{RT_GUIDES_SPECULAR, 0, 0.0f};
    return RT_OK;
}

int rt_camera_progressive_accumulate_specular(rt_camera* cam, rt_history* h, const rt_guide_options* guide_options_,
                                              const rt_specular_temporal_options* options, int32_t commit, uint8_t* rgb,
                                              float* radiance, float* variance_out, float* length_out, float* weight_out,
                                              uint8_t* kind_out) {
    if (!h) return set_error(RT_ERR_INVALID, "null history");
    std::lock_guard<std::mutex> hlock(h->mu);
    return camera_call(cam, [&] {
        const std::string who = "rt_camera_progressive_accumulate_specular";
        const TsOpts o = ts_resolve(options, who);
        const TpSessionChain sc{rs_guide_options(guide_options_, who), o.through, o.point_pixels, kind_out};
        tp_session(cam, h, who, o.base, commit, rgb, radiance, variance_out, length_out, weight_out, &sc);
    });
}

int rt_temporal_accumulate_specular(
    int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position,
    const float* distance, const int32_t* object, const float* chain_normal, const float* chain_position,
    const float* chain_distance, const int32_t* chain_object, const int32_t* chain, const rt_view* view,
    const float* radiance, const int32_t* px_samples, int32_t samples, const float* variance, const rt_view* prev_view,
    const rt_region* prev_region, const float* prev_normal, const float* prev_position, const float* prev_distance,
    const int32_t* prev_object, const float* prev_chain_normal, const float* prev_chain_position,
    const float* prev_chain_distance, const int32_t* prev_chain_object, const int32_t* prev_chain,
    const float* prev_radiance, const float* prev_variance, const float* prev_length, const uint8_t* reusable,
    const uint8_t* through, int32_t n_objects, const rt_specular_temporal_options* options, float* radiance_out,
    float* variance_out, float* length_out, float* weight_out, uint8_t* rgb_out, uint8_t* kind_out) {
    return api_guard([&] {
        const std::string who = "rt_temporal_accumulate_specular";
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!normal || !position || !distance || !object || !radiance || !variance)
            throw std::invalid_argument(who + ": normal, position, distance, object, radiance and variance are required");
        if (!chain_normal || !chain_position || !chain_distance || !chain_object || !chain)
            throw std::invalid_argument(who + ": chain_normal, chain_position, chain_distance, chain_object and chain are required");
        if (!view) throw std::invalid_argument(who + ": view is required");
        if (!prev_view || !prev_normal || !prev_position || !prev_distance || !prev_object || !prev_radiance ||
            !prev_variance || !prev_length)
            throw std::invalid_argument(who + ": prev_view, prev_normal, prev_position, prev_distance, prev_object, "
                                              "prev_radiance, prev_variance and prev_length are required");
        const int pc = (prev_chain_normal != nullptr) + (prev_chain_position != nullptr) + (prev_chain_distance != nullptr) +
                       (prev_chain_object != nullptr) + (prev_chain != nullptr);
        if (pc != 0 && pc != 5)
            throw std::invalid_argument(who + ": prev_chain_normal, prev_chain_position, prev_chain_distance, "
                                              "prev_chain_object and prev_chain must be all given or all NULL "
                                              "(NULL: the history holds no chain planes)");
        if (prev_view->width <= 0 || prev_view->height <= 0)
            throw std::invalid_argument(who + ": the previous view's width and height must be positive");
        if (n_objects < 0 || (n_objects > 0 && (!reusable || !through)))
            throw std::invalid_argument(who + ": reusable and through must hold n_objects >= 0 entries");
        if (samples < 0) throw std::invalid_argument(who + ": samples must not be negative");
        const TsOpts o = ts_resolve(options, who);
        tp_explicit(who,
                    TpCall{width, height, samples, n_objects, region, prev_region, view, prev_view,
                           {normal, position, distance, object, chain_normal, chain_position, chain_distance, chain_object, chain},
                           {prev_normal, prev_position, prev_distance, prev_object, prev_chain_normal, prev_chain_position,
                            prev_chain_distance, prev_chain_object, prev_chain},
                           radiance, variance, prev_radiance, prev_variance, prev_length, px_samples, reusable, through,
                           radiance_out, variance_out, length_out, weight_out, rgb_out, kind_out},
                    o.base, o.point_pixels);
    });
}

}  // extern "C"
