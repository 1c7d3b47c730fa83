// C ABI of the progressive session's focused steps (focus.hpp): the selection of the noisiest
// pixels and the step that samples them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pass_host.hpp"

using namespace rt;

extern "C" {

void rt_focus_options_default(rt_focus_options* options) {
    if (options) *options = rt_focus_options{RT_FOCUS_SCORE_VARIANCE, 250, 0.0f, 0};
}

int rt_camera_progressive_focus(rt_camera* cam, int32_t n_samples, const rt_focus_options* options, const float* score,
                                rt_history* h, uint8_t* rgb, float* radiance, int32_t* px_samples, int32_t* px_bounces,
                                uint8_t* selected_out, rt_render_stats* stats, rt_focus_info* info) {
    const std::string who = "rt_camera_progressive_focus";
    rt_focus_options o;
    rt_focus_options_default(&o);
    if (options) o = *options;
    std::unique_lock<std::mutex> hlock;
    if (h && o.source == RT_FOCUS_SCORE_HISTORY) hlock = std::unique_lock<std::mutex>(h->mu);
    return camera_call(cam, [&] {
        // argument errors first, all of them before any device call
        if (n_samples <= 0 || n_samples > 65535)
            throw std::invalid_argument(who + ": n_samples must be in 1..65535 (the pool kernel's 16-bit sample field)");
        if (o.permille < 1 || o.permille > 1000) throw std::invalid_argument(who + ": permille must be in 1..1000");
        if (!(o.min_score >= 0.0f) || !std::isfinite(o.min_score))
            throw std::invalid_argument(who + ": min_score must be finite and not negative");
        if (o.max_pixels < 0) throw std::invalid_argument(who + ": max_pixels must not be negative");
        if (o.source != RT_FOCUS_SCORE_VARIANCE && o.source != RT_FOCUS_SCORE_MAP && o.source != RT_FOCUS_SCORE_HISTORY)
            throw std::invalid_argument(who + ": source must be one of RT_FOCUS_SCORE_*");
        if (o.source == RT_FOCUS_SCORE_MAP && !score) throw std::invalid_argument(who + ": the score map is required");
        if (o.source == RT_FOCUS_SCORE_HISTORY && !h) throw std::invalid_argument(who + ": the history is required");
        // (session_with's checks, with the history's and the sample index's before the device's)
        DevCtx& c = session_host(cam, who, o.source == RT_FOCUS_SCORE_VARIANCE ? 2 : 0);
        DevCtx::ProgSession& P = c.prog;
        const RtCamera& C = cam->build.cam;
        if (o.source == RT_FOCUS_SCORE_HISTORY) {
            const rt_region& r = h->region;
            if (h->views <= 0) throw std::invalid_argument(who + ": the history is empty");
            if (h->device != c.device) throw std::invalid_argument(who + ": the history was committed on another device");
            if (h->width != C.width || h->height != C.height || r.x != P.region.x || r.y != P.region.y ||
                r.width != P.region.width || r.height != P.region.height)
                throw std::invalid_argument(who + ": the history's last committed region and image size are not the session's");
        }
        if ((long long)C.n_samples + P.focus_done + n_samples > (long long)INT32_MAX)
            throw std::invalid_argument(who + ": the sample index would exceed INT32_MAX");
        session_on_device(c, who);
        const hipStream_t stream = nullptr;
        const int len = n_samples;
        rt_focus_info fi{};
        fi.active = P.n_act;
        fi.first_sample = C.n_samples + P.focus_done;
        if (P.n_act > 0) {  // (a finished session has nothing to select)
            c.prog_focus_alloc();
            long long k = ((long long)P.n_act * o.permille + 999) / 1000;
            if (o.max_pixels > 0) k = std::min<long long>(k, o.max_pixels);
            FocusArgs a{};
            a.act = P.d_act;
            a.n_act = (int32_t)P.n_act;
            a.k = (uint32_t)k;
            std::memcpy(&a.min_bits, &o.min_score, sizeof a.min_bits);
            if (o.min_score == 0.0f) a.min_bits = 0u;  // (-0)
            a.state = P.d_state;
            a.plane = nullptr;
            if (o.source == RT_FOCUS_SCORE_MAP) {
                hip_check(hipMemcpyAsync(P.d_fmap, score, (size_t)P.region.width * P.region.height * sizeof(float),
                                         hipMemcpyHostToDevice, stream),
                          "hipMemcpyAsync");
                a.plane = P.d_fmap;
            } else if (o.source == RT_FOCUS_SCORE_HISTORY) {
                a.plane = h->side[h->front].var;
            }
            a.tiles_x = std::max((P.region.width + kTile - 1) / kTile, 1);
            a.w = P.region.width, a.h = P.region.height;
            a.x0 = P.region.x, a.y0 = P.region.y, a.pitch = C.width;
            a.key = P.d_fkey;
            a.words = P.d_fwords;
            a.list = P.d_focus;
            a.mask = selected_out ? P.d_fmask.p : nullptr;
            if (selected_out)
                hip_check(hipMemsetAsync(P.d_fmask, 0, (size_t)C.width * C.height, stream), "hipMemsetAsync");
            hip_check(hipEventRecord(P.fev[0], stream), "hipEventRecord");
            hip_check(launch_focus_select(a, stream), "focus kernels launch");
            hip_check(hipEventRecord(P.fev[1], stream), "hipEventRecord");
            // the one host sync of the selection: the launch plan needs the count (as prog_read)
            hip_check(hipMemcpyAsync(P.h_fwords, P.d_fwords, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                      "hipMemcpyAsync");
            hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
            hip_check(hipEventElapsedTime(&fi.select_ms, P.fev[0], P.fev[1]), "hipEventElapsedTime");
            fi.selected = P.h_fwords[kFocusSelected];
            fi.eligible = P.h_fwords[kFocusEligible];
            std::memcpy(&fi.threshold, &P.h_fwords[kFocusThreshold], sizeof fi.threshold);
            if (fi.selected > 0) {
                cam->last = &c;
                cam->multi.clear();
                const ProgStep step{P.d_focus, (long)fi.selected, fi.first_sample, len};
                c.launch(P.region, 0, 1, P.precision, cam->traversal, 0, P.d_rgb, P.d_rad, P.d_pxs, P.d_pxb, 0, stream,
                         &step);
                c.prog_read(stream);
                P.focus_done += len;
                P.focused = true;
                ++P.steps;
            }
        } else if (selected_out) {
            c.prog_focus_alloc();
            hip_check(hipMemsetAsync(P.d_fmask, 0, (size_t)C.width * C.height, stream), "hipMemsetAsync");
        }
        fi.focus_done = P.focus_done;
        if (info) *info = fi;
        DevCtx::stats_from_words(P.words, stats);  // throws the render errors of the samples kept
        prog_copy_out(c, rgb, P.d_rgb, 3, stream);
        prog_copy_out(c, radiance, P.d_rad, 3 * sizeof(float), stream);
        prog_copy_out(c, px_samples, P.d_pxs, sizeof(int32_t), stream);
        prog_copy_out(c, px_bounces, P.d_pxb, sizeof(int32_t), stream);
        prog_copy_out(c, selected_out, P.d_fmask, 1, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
}

}  // extern "C"
