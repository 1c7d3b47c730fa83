"""Record the frame passes' argument errors (tests/pass_error_cases.py) from the build in this
tree: pass_errors.json on any machine, pass_errors_session.json (--session) on one with a GPU.

Run it on the commit whose behaviour is to be pinned, BEFORE a change to the ABI layer; every row
must end in RT_ERR_INVALID - one that reaches a device is a finding, not a row to leave out.

    python tests/golden/make_pass_errors.py [--session] [--out DIR]
"""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT / "mcp-raytracer_amd"))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--session", action="store_true", help="the rows that need an open session (a GPU)")
    ap.add_argument("--out", default=str(HERE))
    a = ap.parse_args()
    import pass_error_cases as pc
    import raytracer_amd as rt

    if a.session:
        env = pc.SessionEnv(rt)
        rows = [(cid, *env.call(e, entry, ov)) for cid, e, entry, ov in pc.session_cases()]
        env.close()
        name = "pass_errors_session.json"
    else:
        env = pc.Env(rt)
        rows = [(cid, *env.call(entry, ov)) for cid, entry, ov in pc.cases()]
        name = "pass_errors.json"
    bad = [r for r in rows if r[1] != 1]
    for r in bad:
        print("NOT RT_ERR_INVALID:", r)
    if bad:
        sys.exit(1)
    out = {"build_id": rt.build_id(), "rows": [{"id": i, "code": c, "message": m} for i, c, m in rows]}
    Path(a.out, name).write_text(json.dumps(out, indent=1) + "\n")
    print(f"{name}: {len(rows)} rows from build {out['build_id']}")


if __name__ == "__main__":
    main()
