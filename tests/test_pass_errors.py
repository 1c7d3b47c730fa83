"""The frame passes' argument errors, replayed against fixtures recorded before the ABI layer was
split by pass (tests/golden/make_pass_errors.py): the return code and the WHOLE rt_last_error text
of every row - which error wins when a call has two faults included - and the build lists."""
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pass_error_cases as pc  # noqa: E402


def _fixture(name):
    rows = json.loads((pc.GOLDEN / name).read_text())["rows"]
    return {r["id"]: (r["code"], r["message"]) for r in rows}


def test_pass_argument_errors_are_the_recorded_ones_without_a_device(rt):
    from raytracer_amd import _lib
    want = _fixture("pass_errors.json")
    cases = pc.cases()
    assert sorted(want) == sorted(c[0] for c in cases)          # no row dropped, none unrecorded
    assert {code for code, _ in want.values()} == {_lib.RT_ERR_INVALID}
    entries = {cid.split(":")[0] for cid in want if " + " in cid}
    assert entries == set(pc.ENTRIES), "a precedence row for every entry"
    env = pc.Env(rt)
    got = {cid: env.call(entry, ov) for cid, entry, ov in cases}
    diff = {cid: (got[cid], want[cid]) for cid in want if got[cid] != want[cid]}
    assert not diff, diff


@pytest.mark.gpu
def test_session_argument_errors_are_the_recorded_ones(rt, gpu):
    from raytracer_amd import _lib
    want = _fixture("pass_errors_session.json")
    cases = pc.session_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    assert {code for code, _ in want.values()} == {_lib.RT_ERR_INVALID}
    env = pc.SessionEnv(rt)
    try:
        got = {cid: env.call(e, entry, ov) for cid, e, entry, ov in cases}
    finally:
        env.close()
    diff = {cid: (got[cid], want[cid]) for cid in want if got[cid] != want[cid]}
    assert not diff, diff


def test_every_source_is_in_the_build_lists(rt):
    """The build id hashes _UNITS and _HEADERS: a file missing from them is a stale library reused."""
    from raytracer_amd import _build
    units = sorted(p.name for p in _build.CSRC.iterdir() if p.suffix in (".hip", ".cpp"))
    headers = sorted(p.name for p in _build.CSRC.iterdir() if p.suffix == ".hpp")
    assert units == sorted(u[0] for u in _build._UNITS)
    assert headers == sorted(_build._HEADERS)
    api = {u[0]: u[1:] for u in _build._UNITS if u[0].startswith("api_") or u[0] in ("rt_api.cpp", "pass_host.cpp")}
    # the ABI units share rt_api.cpp's flags: their host arithmetic must not be contracted
    assert len(api) == 6 and all(v == (["-ffp-contract=off", "-x", "hip"], True) for v in api.values())
