"""The quad tail mode of the sphere / box BVH preset with Marble textures (kernel.hip bvh_quad_tail; the showcase
scene, C3), on a real MI355X. The other cases run the same checks on instances that keep the plain loop.

Once the rays of a bvh_hit call that are still traversing fit the call's host quads, each is traversed by the
four lanes of a quad, one BVH4 child slot per lane. The mode changes no bit: every case here is compared with
the CPU oracle bit for bit, with the mode on (the default) and off (RT_OPT_TUNE bits 13-15 = 1).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QUAD_OFF = 1 << 13  # RT_OPT_TUNE bits 13-15 = 1: the plain loop only
QUAD_8 = 4 << 13    # at most 8 rays in quad mode: waves hand over later


def gpu_render(rt, scene, camera, params, tune=0):
    with rt.options(tune=tune):
        ds = rt.DeviceScene(scene)
        try:
            img, st = ds.render(camera, params)
        finally:
            ds.close()
    return img, st


# --- device KAT: the quad's key, rank and push step beside the plain loop's --------------------------------
EMPTY = 0xFFFFFFFF


def _kat_cases():
    """(n, 40) float32 cases for rt_device_kat op 5 and, per case, a label."""
    rng = np.random.default_rng(20240613)
    cases, labels = [], []

    def case(lo, hi, o, d, tmin=0.001, tmax=np.inf, closest=np.inf, prune=0.0, delta=0.0, ids=(11, 22, 33, 44), label=""):
        a = np.zeros(40, dtype=np.float32)
        lo = np.asarray(lo, dtype=np.float32).reshape(4, 3)
        hi = np.asarray(hi, dtype=np.float32).reshape(4, 3)
        for ax in range(3):
            a[4 * ax:4 * ax + 4] = lo[:, ax]
            a[12 + 4 * ax:16 + 4 * ax] = hi[:, ax]
        a[24:28] = np.asarray(ids, dtype=np.uint32).view(np.float32)
        a[28:31], a[31:34] = o, d
        a[34], a[35], a[36], a[37], a[38] = tmin, tmax, closest, prune, delta
        cases.append(a)
        labels.append(label)

    def boxes(n_empty=0):
        c = rng.uniform(-4, 4, (4, 3))
        h = rng.uniform(0.2, 2.5, (4, 3))
        lo, hi = c - h, c + h
        for s in rng.permutation(4)[:n_empty]:  # an empty slot: the inverted infinite box (lower.cpp)
            lo[s], hi[s] = np.inf, -np.inf
        return lo, hi

    signs = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for rep in range(12):  # random nodes and rays, all eight direction-sign combinations, 0-3 empty slots
        for s in signs:
            lo, hi = boxes(n_empty=rep % 4)
            o = rng.uniform(-6, 6, 3)
            d = np.asarray(s) * rng.uniform(0.05, 1.0, 3)
            prune = float(rep % 2)
            case(lo, hi, o, d, closest=np.inf if rep % 3 else rng.uniform(1, 8), prune=prune, delta=1e-4 * prune,
                 tmax=np.inf if rep % 5 else 9.0, label=f"random rep {rep} signs {s}")
    for s in signs:  # the origin inside two and inside four child boxes: keys tie at t_min
        for inside in (2, 4):
            lo, hi = boxes()
            o = rng.uniform(-1, 1, 3)
            for k in rng.permutation(4)[:inside]:
                lo[k], hi[k] = o - rng.uniform(0.5, 2, 3), o + rng.uniform(0.5, 2, 3)
            for prune in (0.0, 1.0):
                case(lo, hi, o, np.asarray(s) * rng.uniform(0.1, 1.0, 3), prune=prune, delta=1e-4 * prune,
                     label=f"origin inside {inside}, signs {s}, prune {prune}")
    for s in signs:  # slabs with planes at +-inf: (+-inf - o) * inv = +-inf, never NaN
        lo, hi = boxes(n_empty=1)
        for k in range(4):
            ax = int(rng.integers(0, 3))
            if np.isfinite(lo[k, 0]):
                lo[k, ax], hi[k, ax] = -np.inf, np.inf
        case(lo, hi, rng.uniform(-3, 3, 3), np.asarray(s) * rng.uniform(0.1, 1.0, 3), label=f"infinite slabs, signs {s}")
    for s in signs:  # a closest that prunes some children: boxes strung along the ray
        d = np.asarray(s) * np.asarray([0.6, 0.5, 0.62])
        o = rng.uniform(-1, 1, 3)
        ts = np.asarray([2.0, 4.0, 6.0, 8.0])[rng.permutation(4)]
        lo = np.stack([o + t * d - 0.4 for t in ts])
        hi = np.stack([o + t * d + 0.4 for t in ts])
        for closest in (1.0, 3.0, 5.0, 7.0, 20.0):
            case(lo, hi, o, d, closest=closest, prune=1.0, delta=1e-4, label=f"closest {closest} prunes, signs {s}")
            case(lo, hi, o, d, closest=closest, prune=0.0, label=f"closest {closest}, not prunable, signs {s}")
    return np.stack(cases), labels


def test_quad_step_equals_the_plain_step(rt):
    # quad_child_key / quad_sort_push on 16 quads a block against child_keys4_nf, the 5-comparator network and
    # the pushes of bvh_run on the same inputs: keys bit for bit, sp, the stack's keys position by position, the
    # entries as a set, and the next node. Children with EQUAL keys may come in another order than the
    # network leaves them (it is not a stable sort; kernel.hip quad_sort_push), so the node ids are compared
    # exactly against the quad's documented rule (nearest first, ties to the lower slot) and as a multiset of
    # (key, node) pairs against the plain step; with distinct keys the two orders are the same.
    cases, labels = _kat_cases()
    out = rt.device_kat_quad(cases)
    assert out.shape == (len(cases), 24)
    n_ties = n_pruned = n_empty_nodes = 0
    for a, o, label in zip(cases, out, labels):
        qk, pk = o[0:4], o[4:8]
        assert (qk == pk).all(), (label, qk, pk)
        q_sp, q_next, q_nodes, q_t = int(o[8]), int(o[9]), o[10:13], o[13:16]
        p_sp, p_next, p_nodes, p_t = int(o[16]), int(o[17]), o[18:21], o[21:24]
        keys = qk.view(np.float32)
        ids = a[24:28].view(np.uint32)
        vis = [k for k in range(4) if keys[k] != np.inf]
        assert q_sp == p_sp == 1 + max(len(vis) - 1, 0), (label, q_sp, p_sp)
        assert (q_t == p_t).all(), (label, q_t, p_t)  # the same keys at the same stack positions
        order = sorted(vis, key=lambda k: (keys[k], k))  # the quad's rule: nearest first, ties to the lower slot
        if not vis:
            n_empty_nodes += 1
            assert q_next == p_next == EMPTY, label
            assert (q_nodes == 0xDEADBEEF).all() and (p_nodes == 0xDEADBEEF).all(), label
            continue
        assert q_next == ids[order[0]], (label, q_next, order)
        want_nodes = [int(ids[k]) for k in reversed(order[1:])]  # far to near
        want_t = [int(qk[k]) for k in reversed(order[1:])]
        assert [int(v) for v in q_nodes[:len(want_nodes)]] == want_nodes, (label, q_nodes, want_nodes)
        assert [int(v) for v in q_t[:len(want_t)]] == want_t, label
        assert (q_nodes[len(want_nodes):] == 0xDEADBEEF).all() and (q_t[len(want_nodes):] == 0xDEADBEEF).all(), label
        # against the plain step: the same (key, node) pairs; the next node has the least key
        m = len(vis) - 1
        pairs_q = sorted([(int(qk[order[0]]), q_next)] + list(zip(map(int, q_t[:m]), map(int, q_nodes[:m]))))
        p_next_key = int(qk[list(ids).index(p_next)])
        pairs_p = sorted([(p_next_key, p_next)] + list(zip(map(int, p_t[:m]), map(int, p_nodes[:m]))))
        assert pairs_q == pairs_p, (label, pairs_q, pairs_p)
        assert keys[list(ids).index(p_next)] == keys[order[0]], label
        if len(set(float(keys[k]) for k in vis)) == len(vis):
            assert q_next == p_next and (q_nodes == p_nodes).all(), (label, q_nodes, p_nodes)
        else:
            n_ties += 1
        n_pruned += int(a[37] != 0 and len(vis) < int(np.isfinite(a[0:4]).sum()))
    assert n_ties >= 16 and n_pruned >= 8 and n_empty_nodes >= 1, (n_ties, n_pruned, n_empty_nodes)


# --- oracle comparisons: the mode on and off -------------------------------------------------------------------
def _nested_scene(rt):
    # the scene shape of test_gpu_parity.py test_instances_media_and_nested_lists
    b = rt.SceneBuilder()
    white = b.lambertian_from_color((0.7, 0.7, 0.7))
    glass = b.dielectric(1.3)
    light = b.diffuse_light_from_color((5, 5, 5))
    chk = b.lambertian(b.checker(3.0, b.solid((0.9, 0.1, 0.1)), b.checker_from_color(7.0, (0, 0, 1), (1, 1, 0))))
    inner = rt.HittableList()
    inner.add(b.cube((-1, -1, -1), (1, 1, 1), white))
    inner.add(b.sphere((0, 2, 0), 0.7, glass))
    lst = rt.HittableList()
    lst.add(b.translate(b.rotate_y(b.translate(b.list(inner), (0.5, 0, 0)), 33.0), (0, 0, 1)))
    lst.add(b.tri((-3, 0, -3), (3, 0, -3), (0, 3, -3), chk))
    spheres = rt.HittableList()
    for i in range(9):
        spheres.add(b.sphere((i - 4.0, -1.5, 0.5 * (i % 3)), 0.4, white))
    w = rt.HittableList()
    w.add(b.list(lst))
    w.add(b.rotate_y(b.constant_medium_from_color(b.cube((-2, -2, -2), (2, 2, 2), white), 0.3, (0.2, 0.9, 0.3)), 10.0))
    w.add(b.constant_medium(b.bvh(spheres, 0.0, 1.0, axis_seed=77), 2.0, b.solid((0.9, 0.9, 0.9))))
    w.add(b.xy_rect(-5, 5, 3, 6, -6, light))
    w.add(b.moving_sphere((2, 1, 2), (3, 2, 2), 0.0, 1.0, 0.5, b.metal((0.9, 0.8, 0.7), 0.3)))
    cam = rt.Camera.new((0, 3, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.2, 12.0, 0.0, 1.0)
    return b.finish(w), cam, rt.render_params(30, 20, 4, 20, background=(0.5, 0.6, 0.7))


def _preset_case(rt, name, w, h, spp):
    # the preset's scene and camera at w x h (C1's own frame is 16:9: the camera takes the case's aspect)
    cfg = rt.CONFIGS[name]
    scene = rt.Scene.generate(cfg.scene, cfg.scene_seed)
    cam = rt.Camera.new(cfg.look_from, cfg.look_at, cfg.view_up, cfg.vfov, w / h, cfg.aperture, cfg.focus_dist,
                        cfg.time0, cfg.time1)
    return scene, cam, rt.render_params(w, h, spp, cfg.depth, background=cfg.background())


@pytest.mark.parametrize("case", ["C3 48x32x3", "C1 64x42x4", "nested instances"])
def test_mode_on_and_off_match_the_oracle(case, rt, orc):
    if case == "nested instances":
        scene, cam, params = _nested_scene(rt)
    else:
        name, dims = case.split()
        w, h, spp = (int(v) for v in dims.split("x"))
        scene, cam, params = _preset_case(rt, name, w, h, spp)
    want, cnt = orc.render(scene, cam, params)
    for tune in (0, QUAD_OFF, QUAD_8):
        got, st = gpu_render(rt, scene, cam, params, tune)
        np.testing.assert_array_equal(got, want)
        assert st["segments"] == cnt["segments"], tune


@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (4, 4, 1), (17, 1, 1), (9, 7, 4)])
def test_few_lane_waves_match_the_oracle(w, h, spp, rt, orc):
    # waves that start below the mode's limit or cross it: 1, 16 and 17 camera rays, and a ragged 9 x 7 x 4
    cfg = rt.CONFIGS["C3"]
    scene = rt.Scene.generate(cfg.scene, cfg.scene_seed)
    cam = rt.Camera.new(cfg.look_from, cfg.look_at, cfg.view_up, cfg.vfov, w / h, cfg.aperture, cfg.focus_dist,
                        cfg.time0, cfg.time1)
    params = rt.render_params(w, h, spp, cfg.depth, background=cfg.background())
    want, cnt = orc.render(scene, cam, params)
    for tune in (0, QUAD_OFF):
        got, st = gpu_render(rt, scene, cam, params, tune)
        np.testing.assert_array_equal(got, want)  # (W - 1 == 0 or H - 1 == 0 divides by zero on both sides)
        assert st["segments"] == cnt["segments"], tune


def test_frames_in_flight_three_handles(rt, orc):
    # RT_FLAG_FRAMES_IN_FLIGHT renders on three handles of one scene (bench.py's N > 1 step), C3 40 px wide
    cfg = rt.CONFIGS["C3"].scaled(40, 3)
    scene = rt.Scene.generate(cfg.scene, cfg.scene_seed)
    plain = rt.render_params(cfg.width, cfg.height, cfg.spp, cfg.depth, background=cfg.background(), seed=9)
    want, cnt = orc.render(scene, cfg.camera(), plain)
    params = rt.render_params(cfg.width, cfg.height, cfg.spp, cfg.depth, background=cfg.background(), seed=9,
                              frames_in_flight=True)
    handles = [rt.DeviceScene(scene) for _ in range(3)]
    try:
        for ds in handles:
            got, st = ds.render(cfg.camera(), params)
            np.testing.assert_array_equal(got, want)
            assert st["segments"] == cnt["segments"]
    finally:
        for ds in handles:
            ds.close()


# --- not vacuous: the audit build counts quad-mode iterations ------------------------------------------------
_AUDIT_CODE = r'''
import sys
sys.path.insert(0, {root!r})
import raytracinginoneweekendinrust_amd as rt
rt.set_option("tune", {tune})
cfg = rt.CONFIGS["C3"].scaled(64, 4)
scene = rt.Scene.generate(cfg.scene, cfg.scene_seed)
p = rt.render_params(cfg.width, cfg.height, cfg.spp, cfg.depth, background=cfg.background())
ds = rt.DeviceScene(scene)
ds.render(cfg.camera(), p)
ds.close()
'''


def _audit_counters(tune):
    lib = os.path.join(ROOT, "raytracinginoneweekendinrust_amd", "_lib", "librtamd_audit.so")
    assert os.path.exists(lib), "build() makes the audit library"
    r = subprocess.run([sys.executable, "-c", _AUDIT_CODE.format(root=ROOT, tune=tune)], capture_output=True, text=True,
                       env=dict(os.environ, RT_LIBRARY=lib), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for ln in r.stderr.splitlines():
        if ln.startswith('{"') and ln.endswith("}") and "_count\"" in ln or ln.startswith('{"quad_iters'):
            out.update(json.loads(ln))
    return out


def test_the_mode_runs_and_the_traversal_audit_is_clean():
    # C3 64 x 42 x 4 spp on the audit build: every fast traversal replayed by the reference recursion agrees
    # (0 mismatches, 0 out-of-range nodes or stack slots), quad-mode iterations were counted, and none with the
    # mode switched off.
    on = _audit_counters(0)
    assert on["trav_audit_count"] == 0 and on["bounds_audit_count"] == 0 and on["leaf_audit_count"] == 0, on
    assert on["quad_iters"] > 0, on
    off = _audit_counters(QUAD_OFF)
    assert off["trav_audit_count"] == 0 and off["bounds_audit_count"] == 0, off
    assert off["quad_iters"] == 0, off
