"""The inputs of the fp32 per-sample tests, checked on the CPU.

test_fp32_gpu.py allows the GPU's fp32 render D_gpu <= 2 * D_orc + 0.005 * N
samples that disagree with the ref oracle, D_orc being the oracle's own fp32
mode's count (fp32_cases.py). That allowance grows with D_orc, so D_orc is
bounded here: if a scene change makes the reference itself decorrelate in fp32,
this suite says so before the GPU test's allowance quietly grows.
"""
import numpy as np
import pytest

import fp32_cases as fc


@pytest.mark.parametrize("name", fc.case_names())
def test_fp32_oracle_rarely_leaves_the_ref_oracle(rt, oracle, name):
    bound = fc.ORACLE_BOUND.get(name, fc.ORACLE_BOUND_DEFAULT)
    for seed in fc.SEEDS:
        ref, f32 = fc.oracle_pair(oracle, name, seed)
        n = ref["px_bounces"].size
        d_orc = fc.disagreeing(f32["radiance"], f32["px_bounces"], ref)
        print(f"{name} seed {seed}: D_orc {d_orc} of N {n} ({d_orc / n:.4f}), bound {bound}")
        assert ref["width"] == fc.WIDTH and np.all(ref["px_samples"] == 1)
        assert d_orc <= bound * n, (name, seed, d_orc, n)
        assert fc.new_nonfinite(f32["radiance"], ref["radiance"]) == 0


def test_backface_case_shows_back_faces(rt, oracle):
    """The back-face case keeps covering back faces: by the ref oracle's closest
    hit along each pixel's camera ray, at least a quarter of the frame is the
    flipped side of the plane or the quad."""
    sd, ro = fc.case("backface", fc.SEEDS[0])
    share = fc.backface_share(oracle, sd, ro)
    print(f"backface: {share:.3f} of the frame is a back face")
    assert share >= 0.25


def test_matrix_quad_shows_one_side_to_the_camera_and_the_other_to_the_floor(rt, oracle):
    """The matrix's free-standing quad: camera rays see its front only, and rays
    leaving the floor behind it reach its back."""
    sd, ro = fc.case("lambert-sky", fc.SEEDS[0])
    info = oracle.camera_info(sd, ro)
    rays = [oracle.get_ray(sd, ro, i, j, 0) for j in range(info["height"]) for i in range(info["width"])]
    h = oracle.world_hit(sd, [r[0] for r in rays], [r[1] for r in rays])
    quad = (h[:, 0] > 0) & (h[:, 9] == 2)
    assert quad.sum() > 50 and np.all(h[quad, 8] == 1)
    rng = np.random.default_rng(5)
    o = np.stack([rng.uniform(0, 1.5, 400), np.zeros(400), rng.uniform(-1.6, -1.0, 400)], axis=1)
    d = rng.normal(size=(400, 3))
    d[:, 1] = np.abs(d[:, 1])
    h = oracle.world_hit(sd, o, d)
    quad = (h[:, 0] > 0) & (h[:, 9] == 2)
    assert quad.sum() > 20 and np.all(h[quad, 8] == 0)
