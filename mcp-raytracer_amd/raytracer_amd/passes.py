"""The frame passes with explicit buffers, no camera - denoise, reproject, temporal_accumulate and
the latter two through specular chains - and the marshalling they share with the Camera,
History and ProgressiveRender methods (camera.py): regions, views, guide planes, per-object
tables, frames, options and outputs, each in one place.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

_VIEW_KEYS = ("center", "pixel00", "du", "dv")


def _region(region) -> _lib.RtRegion:
    if isinstance(region, dict):
        return _lib.RtRegion(int(region["x"]), int(region["y"]), int(region["width"]), int(region["height"]))
    x, y, w, h = region
    return _lib.RtRegion(int(x), int(y), int(w), int(h))


def _region_ptr(region):
    """rt_region* of a `region` argument (None: NULL, the whole image)."""
    return None if region is None else C.byref(_region(region))


def _host_ptr(buf, nbytes: int, what: str):
    """Writable host pointer for a caller-owned buffer (bytearray / numpy / ctypes)."""
    if buf is None:
        return None, None
    try:
        import numpy as np  # noqa: F401
        if hasattr(buf, "__array_interface__"):
            arr = buf
            if not arr.flags["C_CONTIGUOUS"] or not arr.flags["WRITEABLE"]:
                raise ValueError(f"{what} must be a writable C-contiguous array")
            if arr.nbytes < nbytes:
                raise ValueError(f"{what} is too small: {arr.nbytes} < {nbytes} bytes")
            return C.c_void_p(arr.ctypes.data), arr
    except ImportError:  # pragma: no cover
        pass
    mv = memoryview(buf)
    if mv.readonly or mv.nbytes < nbytes:
        raise ValueError(f"{what} must be writable and hold at least {nbytes} bytes")
    cbuf = (C.c_char * mv.nbytes).from_buffer(buf)
    return C.cast(cbuf, C.c_void_p), cbuf


def _c_view(view) -> _lib.RtView:
    import numpy as np
    v = _lib.RtView()
    for k in _VIEW_KEYS:
        getattr(v, k)[:] = [float(x) for x in np.asarray(view[k], dtype=np.float32)]
    v.width, v.height = int(view["width"]), int(view["height"])
    return v


def _view_dict(v: _lib.RtView) -> dict:
    """An rt_view as Camera.view() returns it."""
    import numpy as np
    d = {k: np.array(list(getattr(v, k)), dtype=np.float32) for k in _VIEW_KEYS}
    d.update(width=int(v.width), height=int(v.height))
    return d


def _denoise_options(levels, sigma_color, sigma_plane) -> _lib.RtDenoiseOptions:
    """rt_denoise_options (a zero field = the default; the library validates the rest)."""
    return _lib.RtDenoiseOptions(int(levels), float(sigma_color), float(sigma_plane))


def _var_call(variance, sigma_color, sigma_variance, variance_out, levels, sigma_plane):
    """Which filter a denoise call runs. Without `variance`: (False, rt_denoise_options) - the
    colour edge-stop, sigma_color 0.5 unless given. With it: (True, rt_denoise_var_options)."""
    if variance is None or variance is False:
        if variance_out is not None:
            raise ValueError("variance_out needs variance=")
        return False, _denoise_options(levels, 0.5 if sigma_color is None else sigma_color, sigma_plane)
    if sigma_color is not None:
        raise ValueError("sigma_color belongs to the colour edge-stop: pass either sigma_color or variance=, not both")
    return True, _lib.RtDenoiseVarOptions(int(levels), float(sigma_variance), float(sigma_plane))


def _hold_entry(lib, name, hold_edges):
    """The entry a camera or session filter call runs and the argument the hold form adds after
    its options: [lib.<name>] without hold_edges (0), else [lib.<name>_hold, hold_k] - the library
    refuses values other than 2 and 4."""
    k = int(hold_edges)
    return [getattr(lib, name)] if k == 0 else [getattr(lib, name + "_hold"), k]


def _guide_options(guides) -> _lib.RtGuideOptions:
    """rt_guide_options of a `guides=` keyword: "first_hit", "specular" (max_bounces 8, max_fuzz 0)
    or a dict of max_bounces / max_fuzz for the specular walk (the library validates the values)."""
    if isinstance(guides, str) and guides == "first_hit":
        return _lib.RtGuideOptions(_lib.GUIDES_FIRST_HIT, 8, 0.0)
    if isinstance(guides, str) and guides == "specular":
        guides = {}
    if not isinstance(guides, dict) or set(guides) - {"max_bounces", "max_fuzz"}:
        raise ValueError('guides must be "first_hit", "specular" or a dict of max_bounces / max_fuzz')
    return _lib.RtGuideOptions(_lib.GUIDES_SPECULAR, int(guides.get("max_bounces", 8)), float(guides.get("max_fuzz", 0.0)))


def _gather_options(guides, plain, specular, point_pixels, through, kind, shape):
    """The options of a Camera / ProgressiveRender call that runs the plain entry without `guides=`
    and the one through specular chains with it: (None, the plain options) or (rt_guide_options,
    the specular options around them, the kind pointer)."""
    if guides is None:
        if kind is not None or point_pixels != 4.0 or through != 15:
            raise ValueError("kind, point_pixels and through need guides=")
        return None, plain
    return _guide_options(guides), specular(plain, float(point_pixels), int(through)), _kind_out(kind, shape)


def _var_out(variance_out, shape):
    """Pointer of the optional caller-owned (H, W) float32 array the filtered variance goes to."""
    import numpy as np
    if variance_out is None:
        return None
    if (not isinstance(variance_out, np.ndarray) or variance_out.dtype != np.float32
            or not variance_out.flags["C_CONTIGUOUS"] or not variance_out.flags["WRITEABLE"]
            or variance_out.size != shape[0] * shape[1]):
        raise ValueError("variance_out must be a writable C-contiguous float32 array of H*W values")
    return variance_out.ctypes.data


def _f32_frame(a, shape, what: str):
    """`a` as a C-contiguous float32 / int32 array of `shape` (no copy when it already is)."""
    import numpy as np
    dtype = np.int32 if what == "object" else np.float32
    arr = np.ascontiguousarray(a, dtype=dtype)
    if arr.size != int(np.prod(shape)):
        raise ValueError(f"{what} must hold {'x'.join(str(v) for v in shape)} values, not {arr.size}")
    return arr.reshape(shape)


def _frame_size(object):
    """(H, W) of a call with explicit buffers: the shape of the new view's object plane."""
    import numpy as np
    obj = np.asarray(object)
    if obj.ndim != 2:
        raise ValueError("object must have shape (H, W)")
    return obj.shape


def _planes(g, h, w, with_chain=False):
    """A view's guide planes (a dict as Camera.render_guides returns it) as the arrays a C entry
    takes, in its order; with_chain: the chain word plane after them."""
    a = [_f32_frame(g["normal"], (h, w, 3), "normal"), _f32_frame(g["position"], (h, w, 3), "position"),
         _f32_frame(g["distance"], (h, w), "distance"), _f32_frame(g["object"], (h, w), "object")]
    if with_chain:
        a.append(_f32_frame(g["chain"], (h, w), "object"))
    return a


def _tables(*tables):
    """The per-object uint8 tables of a call (reusable, or reusable and through): their pointers
    (None: no objects) followed by n_objects, and the arrays to keep alive."""
    import numpy as np
    t = [np.ascontiguousarray(a, dtype=np.uint8).ravel() for a in tables]
    if any(a.size != t[0].size for a in t):
        raise ValueError("reusable and through must hold one entry per object")
    return [a.ctypes.data if a.size else None for a in t] + [int(t[0].size)], t


def _px_samples(px_samples, H, W):
    """The optional per-pixel sample counts as an int32 array of H*W values."""
    import numpy as np
    pxs = None if px_samples is None else np.ascontiguousarray(px_samples, dtype=np.int32)
    if pxs is not None and pxs.size != H * W:
        raise ValueError(f"px_samples must hold {H}x{W} values, not {pxs.size}")
    return pxs


def _denoise_out(src, out):
    """The array a filter call writes: `out` (which may be the input itself) or a copy of the
    input, so the pixels outside the region come back unchanged."""
    import numpy as np
    if out is None:
        return np.array(src, dtype=np.float32, copy=True)
    if (not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]
            or not out.flags["WRITEABLE"] or out.size != src.size):
        raise ValueError("out must be a writable C-contiguous float32 array of the radiance's size")
    return out


def _out_array(a, dtype, shape, what: str):
    """Pointer of an optional caller-owned output array of `shape` (any shape of that size)."""
    import numpy as np
    if a is None:
        return None
    if (not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]
            or a.size != int(np.prod(shape))):
        raise ValueError(f"{what} must be a writable C-contiguous {np.dtype(dtype).name} array of "
                         f"{'x'.join(str(v) for v in shape)} values")
    return a.ctypes.data


def _f32_outs(H, W, **outs):
    """Pointers of the optional (H, W) float32 outputs, named by keyword."""
    import numpy as np
    return [_out_array(a, np.float32, (H, W), what) for what, a in outs.items()]


def _kind_out(kind, shape):
    """Pointer of the optional caller-owned (H, W) uint8 array the kind plane goes to."""
    import numpy as np
    return _out_array(kind, np.uint8, shape, "kind")


def _as_frame(a, H, W):
    """A call's result as a (H, W, 3) array: `a` itself when it has that shape."""
    return a if a.shape == (H, W, 3) else a.reshape(H, W, 3)


def _session_frame(cam, rgb, radiance, what="rgb"):
    """The full-frame outputs of a session method: (u8 pointer, radiance pointer, the radiance
    array - a new zero one without `radiance` -, keep-alive)."""
    import numpy as np
    if radiance is None:
        radiance = np.zeros((cam.image_height, cam.image_width, 3), np.float32)
    ptr, k0 = _host_ptr(rgb, cam.byte_length, what)
    rptr, k1 = _host_ptr(radiance, cam.byte_length * 4, "radiance")
    return ptr, rptr, radiance, (k0, k1)


def _session_result(cam, radiance):
    """What a session method returns: its radiance buffer, as (H, W, 3) when it is a float32 array."""
    import numpy as np
    if isinstance(radiance, np.ndarray) and radiance.dtype == np.float32:
        return _as_frame(radiance, cam.image_height, cam.image_width)
    return radiance


def denoise(radiance, normal, position, distance, object, region=None, *, levels=4, sigma_color=None,
            sigma_plane=0.01, rgb=None, out=None, variance=None, sigma_variance=2.0, variance_out=None, chain=None,
            hold=None):
    """rt_denoise: the guided edge-avoiding a-trous filter of a frame with explicit guides (as
    Camera.render_guides returns them), no camera. radiance / normal / position: float32
    (H, W, 3); distance float32, object int32: (H, W). Returns the filtered radiance (H, W, 3) -
    a new array, or `out` (which may be `radiance` itself); only the region is filtered. `rgb`
    (optional caller-owned u8 H*W*3) receives the region's u8. Equals tests/denoise_ref.py in
    every bit. sigma_color defaults to 0.5.

    `variance` (float32 (H, W): the variance of each pixel's mean illuminance, as
    ProgressiveRender.variance returns it) selects the variance-guided filter
    (rt_denoise_variance, tests/denoise_var_ref.py) with `sigma_variance` in place of
    sigma_color; `variance_out` (optional float32 (H, W)) then receives the region's filtered
    variance. Passing sigma_color together with variance raises ValueError. `chain` is accepted
    and ignored, so denoise(radiance, **cam.render_guides(through_specular=True)) works.

    `hold` (uint8 or bool (H, W), e.g. cam.render_coverage()["mixed"]; rt_denoise_hold,
    rt_denoise_variance_hold) marks pixels the filter copies through: they serve as taps as ever,
    and their colour, u8 and variance_out are their inputs (the variance sanitised: negative and
    non-finite values are 0)."""
    import numpy as np
    rad = np.asarray(radiance)
    if rad.ndim != 3 or rad.shape[2] != 3:
        raise ValueError("radiance must have shape (H, W, 3)")
    H, W = rad.shape[:2]
    rad = _f32_frame(rad, (H, W, 3), "radiance")
    g = _planes(dict(normal=normal, position=position, distance=distance, object=object), H, W)
    res = _denoise_out(rad, out)
    uptr, _k = _host_ptr(rgb, H * W * 3, "rgb")
    rptr = _region_ptr(region)
    guided, opts = _var_call(variance, sigma_color, sigma_variance, variance_out, levels, sigma_plane)
    mask = None if hold is None else np.ascontiguousarray(hold, dtype=np.uint8)
    if mask is not None and mask.size != H * W:
        raise ValueError(f"hold must hold {H}x{W} values, not {mask.size}")
    held = [] if mask is None else [mask.ctypes.data]
    lib, suffix = _lib.load(), "" if mask is None else "_hold"
    if guided:
        var = _f32_frame(variance, (H, W), "variance")
        _lib.check(getattr(lib, "rt_denoise_variance" + suffix)(
            W, H, rptr, C.byref(opts), rad.ctypes.data, var.ctypes.data, *[a.ctypes.data for a in g], *held,
            res.ctypes.data, _var_out(variance_out, (H, W)), uptr))
    else:
        _lib.check(getattr(lib, "rt_denoise" + suffix)(W, H, rptr, C.byref(opts), rad.ctypes.data,
                                                       *[a.ctypes.data for a in g], *held, res.ctypes.data, uptr))
    return _as_frame(res, H, W)


def _reproject_options(normal_min, sigma_plane, min_weight, history_samples) -> _lib.RtReprojectOptions:
    """rt_reproject_options (a zero field = the default; the library validates the rest)."""
    return _lib.RtReprojectOptions(float(normal_min), float(sigma_plane), float(min_weight), float(history_samples))


def _temporal_options(normal_min, sigma_plane, min_weight, max_history, filter_levels, sigma_variance):
    """rt_temporal_options (a zero field = the default; the library validates the rest)."""
    return _lib.RtTemporalOptions(float(normal_min), float(sigma_plane), float(min_weight), float(max_history),
                                  int(filter_levels), float(sigma_variance))


def _reproject_frames(H, W, radiance, px_samples, samples, rgb, out, history_out, weight_out):
    """The new frame's side of a reproject call: the entry's trailing arguments (fresh radiance,
    px_samples, scalar samples, history, weight, blend, rgb), the array the call returns - the
    blend, or without `radiance` the history: then out / rgb / px_samples raise - and a keep-alive."""
    import numpy as np
    if radiance is None and (out is not None or rgb is not None or px_samples is not None):
        raise ValueError("out, rgb and px_samples need radiance=")
    rad = None if radiance is None else _f32_frame(radiance, (H, W, 3), "radiance")
    pxs = _px_samples(px_samples, H, W)
    res = None if rad is None else _denoise_out(rad, out)
    hist = np.zeros((H, W, 3), np.float32) if history_out is None and rad is None else history_out
    uptr, keep = _host_ptr(rgb, H * W * 3, "rgb")
    args = [None if rad is None else rad.ctypes.data, None if pxs is None else pxs.ctypes.data,
            0 if samples is None else int(samples), _out_array(hist, np.float32, (H, W, 3), "history_out"),
            *_f32_outs(H, W, weight_out=weight_out), None if res is None else res.ctypes.data, uptr]
    return args, _as_frame(hist if res is None else res, H, W), (rad, pxs, keep)


def _accumulate_frames(H, W, radiance, variance, px_samples, samples, rgb, out, variance_out, length_out, weight_out):
    """The new frame's side of an accumulate call: the fresh frame's arguments (radiance,
    px_samples, scalar samples, variance), the outputs' (radiance, variance, length, weight, rgb),
    the array the call returns and a keep-alive."""
    rad = _f32_frame(radiance, (H, W, 3), "radiance")
    var = _f32_frame(variance, (H, W), "variance")
    pxs = _px_samples(px_samples, H, W)
    res = _denoise_out(rad, out)
    uptr, keep = _host_ptr(rgb, H * W * 3, "rgb")
    fresh = [rad.ctypes.data, None if pxs is None else pxs.ctypes.data, 0 if samples is None else int(samples),
             var.ctypes.data]
    outs = [res.ctypes.data, *_f32_outs(H, W, variance_out=variance_out, length_out=length_out, weight_out=weight_out),
            uptr]
    return fresh, outs, _as_frame(res, H, W), (rad, var, pxs, keep)


def _views(first, chain, prev_view, prev_first, prev_chain):
    """Both views' side of a call with explicit buffers: (H, W, Hp, Wp, the new view's plane
    pointers, the previous view's, the previous rt_view, keep-alive). chain / prev_chain: the guides
    through the chain (None: a plain call; prev_chain False: five NULL planes)."""
    H, W = _frame_size(first["object"])
    Wp, Hp = int(prev_view["width"]), int(prev_view["height"])
    pv = _c_view(prev_view)
    g = _planes(first, H, W) + (_planes(chain, H, W, True) if chain is not None else [])
    held = prev_chain is not None and prev_chain is not False
    pg = _planes(prev_first, Hp, Wp) + (_planes(prev_chain, Hp, Wp, True) if held else [])
    ptrs = lambda planes: [a.ctypes.data for a in planes]  # noqa: E731
    return H, W, Hp, Wp, ptrs(g), ptrs(pg) + ([None] * 5 if prev_chain is False else []), pv, (g, pg)


def _reproject(prev_radiance, prev_view, prev_first, prev_chain, view, first, chain, tables, opts, kind, region, prev_region,
               **frames):
    """reproject() (view, chain, prev_chain, kind: None) and reproject_specular()."""
    spec = chain is not None
    H, W, Hp, Wp, g, pg, pv, _keep = _views(first, chain, prev_view, prev_first, prev_chain)
    prad = _f32_frame(prev_radiance, (Hp, Wp, 3), "prev_radiance")
    tabs, _keep2 = _tables(*tables)
    args, res, _keep3 = _reproject_frames(H, W, **frames)
    fn = _lib.load().rt_reproject_specular if spec else _lib.load().rt_reproject
    _lib.check(fn(W, H, _region_ptr(region), *g, *([C.byref(_c_view(view))] if spec else []), C.byref(pv),
                  _region_ptr(prev_region), prad.ctypes.data, *pg, *tabs, C.byref(opts), *args,
                  *([_kind_out(kind, (H, W))] if spec else [])))
    return res


def reproject(prev_radiance, prev_view, prev_guides, *, normal, position, distance, object, reusable, region=None,
              prev_region=None, radiance=None, px_samples=None, samples=None, rgb=None, out=None, history_out=None,
              weight_out=None, normal_min=0.9, sigma_plane=0.01, min_weight=0.25, history_samples=32.0):
    """rt_reproject: a previous view's frame reprojected into a new view, explicit buffers, no
    camera. prev_radiance float32 (Hp, Wp, 3), prev_view as Camera.view() and prev_guides as
    Camera.render_guides() of the previous camera; normal / position / distance / object: the new
    view's guides (pass **cam.render_guides()); reusable: uint8 per object, as
    Camera.reusable_objects(). With a fresh `radiance` (float32 (H, W, 3)) and its sample counts
    (`px_samples` int32 (H, W), or one scalar `samples`) returns the blend (H, W, 3) - a new array,
    or `out` - and `rgb` (optional u8 H*W*3) receives its u8; without, returns the history.
    `history_out` (float32 (H, W, 3)) and `weight_out` (float32 (H, W)) are optional; only the
    region is written. Equals tests/reproject_ref.py in every bit."""
    return _reproject(prev_radiance, prev_view, prev_guides, None, None,
                      dict(normal=normal, position=position, distance=distance, object=object), None, (reusable,),
                      _reproject_options(normal_min, sigma_plane, min_weight, history_samples), None, region, prev_region,
                      radiance=radiance, px_samples=px_samples, samples=samples, rgb=rgb, out=out,
                      history_out=history_out, weight_out=weight_out)


def reproject_specular(prev_radiance, prev_view, prev_first, prev_chain, view, first, chain, reusable, through, *,
                       region=None, prev_region=None, radiance=None, px_samples=None, samples=None, rgb=None, out=None,
                       history_out=None, weight_out=None, kind=None, normal_min=0.9, sigma_plane=0.01, min_weight=0.25,
                       history_samples=32.0, point_pixels=4.0):
    """rt_reproject_specular: reproject() through specular chains, explicit buffers, no camera.
    first / prev_first: the new and the previous view's first-hit guides as Camera.render_guides()
    returns them; chain / prev_chain: their guides through the chain, render_guides(
    through_specular=True) of one max_bounces / max_fuzz (with "chain"); view: the new camera's
    Camera.view(); reusable / through: uint8 per object, as Camera.reusable_objects() and
    Camera.through_objects(). A pixel whose chain has length 0 is reproject()'s; a pixel that shows a
    lambert or light surface through a chain finds its history at the chain's virtual point. `kind`
    (optional uint8 (H, W)) receives 0 no history, 1 first hit, 2 chain. Everything else as
    reproject(). Equals tests/specular_reproject_ref.py in every bit."""
    opts = _lib.RtSpecularReprojectOptions(_reproject_options(normal_min, sigma_plane, min_weight, history_samples),
                                           float(point_pixels), 0)
    return _reproject(prev_radiance, prev_view, prev_first, prev_chain, view, first, chain, (reusable, through), opts, kind,
                      region, prev_region, radiance=radiance, px_samples=px_samples, samples=samples, rgb=rgb, out=out,
                      history_out=history_out, weight_out=weight_out)


def _accumulate(prev_radiance, prev_variance, prev_length, prev_view, prev_first, prev_chain, view, first, chain, tables,
                opts, kind, region, prev_region, **frames):
    """temporal_accumulate() (view, chain, kind: None; prev_chain: None) and
    temporal_accumulate_specular() (prev_chain False: the history holds no chain planes)."""
    spec = chain is not None
    H, W, Hp, Wp, g, pg, pv, _keep = _views(first, chain, prev_view, prev_first, prev_chain)
    prev = [_f32_frame(prev_radiance, (Hp, Wp, 3), "prev_radiance"), _f32_frame(prev_variance, (Hp, Wp), "prev_variance"),
            _f32_frame(prev_length, (Hp, Wp), "prev_length")]
    tabs, _keep2 = _tables(*tables)
    fresh, outs, res, _keep3 = _accumulate_frames(H, W, **frames)
    fn = _lib.load().rt_temporal_accumulate_specular if spec else _lib.load().rt_temporal_accumulate
    _lib.check(fn(W, H, _region_ptr(region), *g, *([C.byref(_c_view(view))] if spec else []), *fresh, C.byref(pv),
                  _region_ptr(prev_region), *pg, *[a.ctypes.data for a in prev], *tabs, C.byref(opts), *outs,
                  *([_kind_out(kind, (H, W))] if spec else [])))
    return res


def temporal_accumulate(prev_radiance, prev_variance, prev_length, prev_view, prev_guides, *, normal, position, distance,
                        object, reusable, radiance, variance, px_samples=None, samples=None, region=None,
                        prev_region=None, rgb=None, out=None, variance_out=None, length_out=None, weight_out=None,
                        filter_levels=0, sigma_variance=2.0, normal_min=0.9, sigma_plane=0.01, min_weight=0.25,
                        max_history=256.0):
    """rt_temporal_accumulate: one accumulation step with explicit buffers, no camera and no
    History. prev_radiance float32 (Hp, Wp, 3), prev_variance / prev_length float32 (Hp, Wp),
    prev_view as Camera.view() and prev_guides as Camera.render_guides() of the previous view;
    normal / position / distance / object: the new view's guides; reusable: uint8 per object;
    radiance float32 (H, W, 3), variance float32 (H, W) and the sample counts (`px_samples` int32
    (H, W), or one scalar `samples`) of the fresh frame. Returns the accumulated radiance (H, W, 3)
    - `out`, or a new array that holds the fresh frame outside the region - filtered by the
    variance-guided filter when filter_levels > 0; `rgb`, `variance_out`, `length_out` and
    `weight_out` are optional; only the region is written. Equals tests/temporal_ref.py in every
    bit. Views must be rendered with different seeds."""
    return _accumulate(prev_radiance, prev_variance, prev_length, prev_view, prev_guides, None, None,
                       dict(normal=normal, position=position, distance=distance, object=object), None, (reusable,),
                       _temporal_options(normal_min, sigma_plane, min_weight, max_history, filter_levels, sigma_variance),
                       None, region, prev_region, radiance=radiance, variance=variance, px_samples=px_samples,
                       samples=samples, rgb=rgb, out=out, variance_out=variance_out, length_out=length_out,
                       weight_out=weight_out)


def temporal_accumulate_specular(prev_radiance, prev_variance, prev_length, prev_view, prev_first, prev_chain, view, first,
                                 chain, reusable, through, *, radiance, variance, px_samples=None, samples=None,
                                 region=None, prev_region=None, rgb=None, out=None, variance_out=None, length_out=None,
                                 weight_out=None, kind=None, filter_levels=0, sigma_variance=2.0, normal_min=0.9,
                                 sigma_plane=0.01, min_weight=0.25, max_history=256.0, point_pixels=4.0):
    """rt_temporal_accumulate_specular: temporal_accumulate() through specular chains, explicit
    buffers, no camera and no History. first / prev_first: the new and the previous view's first-hit
    guides as Camera.render_guides() returns them; chain / prev_chain: their guides through the
    chain, render_guides(through_specular=True) of one max_bounces / max_fuzz (with "chain");
    prev_chain=None: the history holds no chain planes (every pixel behind a chain starts over);
    view: the new camera's Camera.view(); reusable / through: uint8 per object, as
    Camera.reusable_objects() and Camera.through_objects(). A pixel whose chain has length 0 is
    temporal_accumulate()'s; a pixel that shows a lambert or light surface through a chain finds its
    history - colour, length and variance - at the chain's virtual point. `kind` (optional uint8
    (H, W)) receives 0 no history, 1 first hit, 2 chain. filter_levels > 0 filters with the chain
    guides. Everything else as temporal_accumulate(). Equals tests/specular_temporal_ref.py in every
    bit. Views must be rendered with different seeds."""
    opts = _lib.RtSpecularTemporalOptions(
        _temporal_options(normal_min, sigma_plane, min_weight, max_history, filter_levels, sigma_variance),
        float(point_pixels), 0)
    return _accumulate(prev_radiance, prev_variance, prev_length, prev_view, prev_first,
                       False if prev_chain is None else prev_chain, view, first, chain, (reusable, through), opts, kind,
                       region, prev_region, radiance=radiance, variance=variance, px_samples=px_samples, samples=samples,
                       rgb=rgb, out=out, variance_out=variance_out, length_out=length_out, weight_out=weight_out)
