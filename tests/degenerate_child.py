"""Child process of test_degenerate_abi.py: inputs that used to end the process (a material
that reaches itself, a chain of materials or JSON nested deeper than any stack) go through
the library and the oracle here, so a regression is a failed test and not a dead pytest.

    python degenerate_child.py cycle1 | cycle2 | chain | deep_json

prints one JSON object: for every entry point tried, the message of the error it raised
(null where it returned normally).
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "mcp-raytracer_amd"), str(ROOT / "oracle"), str(ROOT / "tests")]

DEEP = 100000
CHAIN = 100000


def material_scene(kind):
    import degenerate_cases as dc
    sd = dc.base_scene()
    if kind == "cycle1":
        sd["materials"].append({"id": "a", "material": {"type": "mixed", "diff": "a", "spec": "a", "weight": 0.5}})
        first = "a"
    elif kind == "cycle2":
        sd["materials"].append({"id": "a", "material": {"type": "layered", "outer": "glass", "inner": "b"}})
        sd["materials"].append({"id": "b", "material": {"type": "mixed", "diff": "red", "spec": "a", "weight": 0.5}})
        first = "a"
    else:  # acyclic: c0 -> c1 -> ... -> red
        for k in range(CHAIN):
            nxt = f"c{k + 1}" if k + 1 < CHAIN else "red"
            sd["materials"].append({"id": f"c{k}", "material": {"type": "layered", "outer": "glass", "inner": nxt}})
        first = "c0"
    sd["objects"].append({"type": "sphere", "pos": dc.P, "r": 0.35, "material": first})
    return sd, dc.render_options()


def message(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 - the message is the result
        return f"{type(e).__name__}: {e}"
    return None


def materials(kind):
    import pyoracle
    import raytracer_amd as rt
    sd, ro = material_scene(kind)
    return {"lib": message(lambda: rt.create_camera_from_scene_data(sd, ro)),
            "oracle": message(lambda: pyoracle.render(sd, ro)),
            "oracle_fp32": message(lambda: pyoracle.render(sd, ro, precision="fp32"))}


def nested(open_, close, depth):
    return open_ * depth + "1" + close * depth


def deep_json():
    import ctypes as C

    import degenerate_cases as dc
    import raytracer_amd as rt
    from raytracer_amd import _lib
    from raytracer_amd.camera import Camera
    sd, ro = dc.case("base")
    scene = _lib.to_json(sd).decode()
    opts = _lib.to_json(ro).decode()
    assert scene[0] == "{" and opts[0] == "{"

    def junk(text, value):  # the document with a first key "junk" holding `value`
        return ('{"junk":' + value + "," + text[1:]).encode()

    def generate(options):
        out = C.c_void_p()
        lib = _lib.load()
        _lib.check(lib.rt_generate_scene_data(b"spheres", options, C.byref(out)))
        lib.rt_free(out)

    res = {}
    for what, (o, c) in {"arrays": ("[", "]"), "objects": ('{"a":', "}")}.items():
        deep, ok = nested(o, c, DEEP), nested(o, c, 200)
        res[f"{what} scene"] = message(lambda: Camera(junk(scene, deep), opts.encode()))
        res[f"{what} options"] = message(lambda: Camera(scene.encode(), junk(opts, deep)))
        res[f"{what} generate"] = message(lambda: generate(junk('{"count":3,"seed":1}', deep)))
        res[f"{what} scene 200"] = message(lambda: Camera(junk(scene, ok), junk(opts, ok)))
        res[f"{what} generate 200"] = message(lambda: generate(junk('{"count":3,"seed":1}', ok)))
    res["unclosed"] = message(lambda: Camera(("[" * DEEP).encode(), None))
    assert isinstance(rt.build_id(), str)
    return res


if __name__ == "__main__":
    kind = sys.argv[1]
    print(json.dumps(deep_json() if kind == "deep_json" else materials(kind)))
