// The error mapping of the C ABI, written once: api_guard runs an entry's body and maps what it
// throws to (return code, rt_last_error text); the *_call wrappers take an object's lock first.
#pragma once

#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>

#include "dev_ctx.hpp"

namespace rt {

// Sets the calling thread's rt_last_error text and returns `code` (rt_api.cpp).
int set_error(int code, const std::string& msg);

// HIP errors -> RT_ERR_DEVICE, argument errors -> RT_ERR_INVALID, the reference's render errors
// and everything else -> RT_ERR_RENDER.
template <class F>
int api_guard(F&& f) {
    try {
        f();
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

// Runs f under the camera's lock.
template <class F>
int camera_call(rt_camera* cam, F&& f) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    std::lock_guard<std::mutex> lock(cam->mu);
    return api_guard(f);
}

// Runs f under both cameras' locks (one lock when they are the same camera).
template <class F>
int two_camera_call(rt_camera* cam, rt_camera* prev_cam, F&& f) {
    if (!cam || !prev_cam) return set_error(RT_ERR_INVALID, "null camera");
    std::unique_lock<std::mutex> la(cam->mu, std::defer_lock), lb(prev_cam->mu, std::defer_lock);
    if (cam == prev_cam)
        la.lock();
    else
        std::lock(la, lb);
    return api_guard(f);
}

// Runs f under the history's lock.
template <class F>
int history_call(rt_history* h, F&& f) {
    if (!h) return set_error(RT_ERR_INVALID, "null history");
    std::lock_guard<std::mutex> lock(h->mu);
    return api_guard(f);
}

}  // namespace rt
