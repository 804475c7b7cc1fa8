"""A call's result does not depend on the context's history.

One interpreter runs a program of tests/history_model.py on one context (`run`) and every query again on a FRESH context in which only
the state in force has been installed (`expected`; for a call of an accumulation, the accumulation's own begin and calls and nothing
else).  Whatever a query returns -- image, mean and sum bits, hit indices and distance bits, counts and n_active, G-buffer and denoised
bytes, the code of a refusal, scans_executed and kernel_variant -- must be equal bit for bit: STATED TOLERANCE 0.  n_launches is
printed, not compared: the chunk count may follow the device's free memory.

A fresh context is code under test too, so it is not the only reference: every flags-0 render is also held to the oracle's
render_counter, every hit query outside the BVH to the oracle's closest_hits, every step of a plain flags-0 accumulation to the
oracle's render of its total, and every hand-written program holds one featured render that is also held to the numpy model that owns
the feature (path_model.render; the tile equivalence of tests/test_hip_texture.py for the atlas; nmap_model.render for the normal map).

The anchored render is 40 x 26 at 3 spp (history_model.ANCHOR): at 24 x 16 and 2 spp the slowest model call took 0.13 s, so the frame
grew to one of more than 1024 pixels; the model's measured times at that size are in ANCHOR_SECONDS below, 0.44 s at the most.

Device-pointer calls alternate between two torch streams and synchronise after each call, as the header's stream contract asks of
calls on different streams of one context.  Before each operation its text form is printed and flushed: the log of a run that dies
names the operation that was running."""
import re
import sys
import time

import numpy as np
import pytest

import hip_checks as hc
import history_model as hm
from hip_checks import _torch_first  # noqa: F401  (fixture)
from history_model import Op
from spath_amd import capi, view

pytestmark = pytest.mark.gpu

# seconds of the numpy model for the anchored render of each hand-written program (scene, flags), measured on the CPU
ANCHOR_SECONDS = {
    "order_of_5_17[plain]": 0.03, "order_of_5_17[nee]": 0.04, "order_of_5_17[mis]": 0.05, "order_of_5_17[env]": 0.07, "order_of_5_17[tex]": 0.07,
    "order_of_5_17[nmap]": 0.07, "order_of_5_17[widest]": 0.09, "large_small_large[mis]": 0.18, "large_small_large[tex]": 0.19,
    "scene_change_with_tables": 0.44, "same_size_swap": 0.20, "environment_transitions": 0.07, "denoiser_state": 0.05,
    "refusals_change_nothing": 0.07,
}
STAT_KINDS = ("render", "render_camera", "render_device", "render_device_accum", "closest_hit_device", "accum_step", "accum_denoise")
_RAYS, _ORACLE, _EXPECTED, _STREAMS = {}, {}, {}, []


# ---------------------------------------------------------------------------------------------------------------- helpers
def cam_rays(w, h):
    if (w, h) not in _RAYS:
        _RAYS[w, h] = hc.cam_rays(w, h, hm.MOVES)
    return _RAYS[w, h]


def stream(i):
    import torch
    if not _STREAMS:
        _STREAMS.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _STREAMS[i]


def dev(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return d


def host(d):
    return d.cpu().numpy()


def source_triangles(n, n_tris):
    """the idx_source of a hit query with skip=1: a fixed pattern over the triangles, every third ray none"""
    k = np.arange(n, dtype=np.int64)
    return np.where(k % 3 == 0, -1, (k * 7) % n_tris).astype(np.int32)


def noisy_mean(w, h, var):
    rng = np.random.default_rng(1000 * w + h)
    return rng.random((w * h, 3)).astype(np.float32), (rng.random(w * h) * 0.05).astype(np.float32) if var else None


# ---------------------------------------------------------------------------------------------------------------- one call
def _do(c, op, state, out):
    import torch
    k = op.kind
    st = stream(op.stream) if "stream" in op.a else None
    sp = st.cuda_stream if st is not None else 0
    scene_name = state.scene or "room200"
    n = op.w * op.h if "w" in op.a else 0
    if k == "set_scene":
        t, m = hm.scene_data(op.name)
        if op.form == "host":
            c.set_scene(t, m)
        else:
            d_t, d_m = dev(t), dev(m)
            c.set_scene_device(d_t.data_ptr(), d_m.data_ptr(), t.shape[0], sp)
            st.synchronize()
    elif k == "set_table":
        rows = hm.table_data(op.table, scene_name, bool(op.bad))
        if op.form == "host":
            c._set_table(hm.TABLE_SETTER[op.table], rows)
        else:
            d = dev(rows)
            c._set_table_device(hm.TABLE_SETTER[op.table], d.data_ptr(), sp)
            st.synchronize()
    elif k in ("set_env", "set_atlas", "set_nmap"):
        x = hm.env_data(op.map, bool(op.bad)) if k == "set_env" else hm.atlas_data(bool(op.bad)) if k == "set_atlas" else hm.nmap_data()
        if op.form == "host":
            {"set_env": c.set_environment, "set_atlas": c.set_texture, "set_nmap": c.set_normal_map}[k](x)
        else:
            d = dev(x)
            if k == "set_env":
                c.set_environment_device(d.data_ptr(), x.shape[0], sp)
            elif k == "set_atlas":
                c.set_texture_device(d.data_ptr(), x.shape[1], x.shape[0], sp)
            else:
                c.set_normal_map_device(d.data_ptr(), x.shape[1], x.shape[0], sp)
            st.synchronize()
    elif k == "set_lens":
        c.set_lens(*hm.LENSES[op.lens])
    elif k == "render":
        pt = op.mode == "pt"
        r = c.render(cam_rays(op.w, op.h)[1], op.w, op.h, op.spp, seed=op.seed, mode=capi.MODE_PT if pt else capi.MODE_FLAT, flags=op.flags, want_accum=pt)
        out["img"], out["mean"] = r if pt else (r, None)
    elif k == "render_camera":
        out["img"], out["mean"] = c.render_camera(cam_rays(op.w, op.h)[0], op.spp, seed=op.seed, mode=capi.MODE_PT, flags=op.flags, want_accum=True)
    elif k == "render_device":
        pt = op.mode == "pt"
        d_rays = dev(cam_rays(op.w, op.h)[1])
        d_out = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        d_acc = torch.zeros(n * 3, dtype=torch.float32, device="cuda") if pt and op.accum else None
        torch.cuda.synchronize()
        c.render_device(d_rays.data_ptr(), n, op.spp, d_out.data_ptr(), seed=op.seed, mode=capi.MODE_PT if pt else capi.MODE_FLAT, flags=op.flags,
                        image_width=op.w, d_out_accum=d_acc.data_ptr() if d_acc is not None else 0, stream=sp)
        st.synchronize()
        out["img"], out["mean"] = host(d_out).reshape(-1, 4), host(d_acc).reshape(-1, 3) if d_acc is not None else None
    elif k == "render_device_accum":
        d_rays = dev(cam_rays(op.w, op.h)[1])
        d_sum = torch.full((n * 3,), float("nan"), dtype=torch.float32, device="cuda")     # sample_base 0 "ignores d_sum's contents"
        d_out = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        d_mean = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for base, cnt in ((0, op.split), (op.split, op.spp - op.split)):
            c.render_device_accum(d_rays.data_ptr(), n, base, cnt, d_sum.data_ptr(), d_out.data_ptr(), seed=op.seed, flags=op.flags, image_width=op.w,
                                  d_out_mean=d_mean.data_ptr(), stream=sp)
        st.synchronize()
        out["img"], out["mean"], out["sum"] = host(d_out).reshape(-1, 4), host(d_mean).reshape(-1, 3), host(d_sum)
    elif k == "closest_hit_device":
        d_rays = dev(cam_rays(op.w, op.h)[1])
        d_src = dev(source_triangles(n, hm.SCENE_TRIS[scene_name])) if op.skip else None
        d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.closest_hit_device(d_rays.data_ptr(), n, d_idx.data_ptr(), d_dist.data_ptr(), d_src_idx=d_src.data_ptr() if op.skip else 0, flags=op.flags, stream=sp)
        st.synchronize()
        out["idx"], out["dist"] = host(d_idx), host(d_dist)
    elif k == "accum_begin":
        cam, r = cam_rays(op.w, op.h)
        rule = hm.RULES[op.rule] if op.rule >= 0 else None
        if op.src == "cam":
            c.accum_begin(cam=cam, seed=op.seed, flags=op.flags, adaptive=rule)
        else:
            c.accum_begin(rays=r, w=op.w, h=op.h, seed=op.seed, flags=op.flags, adaptive=rule)
    elif k == "accum_step":
        out["img"], out["mean"], out["total"] = c.accum_step(op.n, want_mean=True)
    elif k == "accum_counts":
        out["counts"], out["n_active"] = c.accum_counts()
    elif k == "accum_gbuffer":
        out["gbuf"] = c.accum_gbuffer().view(np.uint32)
    elif k == "accum_denoise":
        out["img"], out["rgb"] = c.accum_denoise(want_rgb=True)
    elif k in ("gbuffer_device", "denoise_device"):
        d_rays = dev(cam_rays(op.w, op.h)[1])
        d_g = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.gbuffer_device(d_rays.data_ptr(), n, d_g.data_ptr(), flags=op.flags if k == "gbuffer_device" else 0, stream=sp)
        if k == "gbuffer_device":
            st.synchronize()
            out["gbuf"] = host(d_g).view(np.uint32)
        else:
            mean, var = noisy_mean(op.w, op.h, op.var)
            d_mean, d_var = dev(mean), dev(var) if op.var else None
            d_rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
            d_rgb = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            c.denoise_device(op.w, op.h, d_mean.data_ptr(), d_g.data_ptr(), d_rgba.data_ptr(), d_var=d_var.data_ptr() if op.var else 0,
                             d_out_rgb=d_rgb.data_ptr(), stream=sp)
            st.synchronize()
            out["img"], out["rgb"] = host(d_rgba).reshape(-1, 4), host(d_rgb).reshape(-1, 3)
    else:
        raise KeyError(k)


def call(c, op, state):
    """op on context c in model state `state` -> {output name: value}; "code" is the status, names with "_" are reported only"""
    out = {}
    try:
        _do(c, op, state, out)
        out["code"] = 0
    except capi.SpathHipError as e:
        code = int(re.search(r"\[(-?\d+)\]", str(e)).group(1))
        if code == -2:                                              # SPHIP_E_DEVICE: nothing more is started on the GPU in this session
            pytest.exit("device error in `%s`: %s" % (op.text(), e), returncode=3)
        return {"code": code}
    if op.kind in STAT_KINDS:
        s = c.stats()
        out["scans"], out["variant"], out["_n_launches"] = s["scans_executed"], s["kernel_variant"], s["n_launches"]
    return {k: v for k, v in out.items() if v is not None}


def context(multi):
    return capi.Context.multi([0, 0]) if multi else capi.Context(0)


# ---------------------------------------------------------------------------------------------------------------- the two roles
def expected(op, state, multi=False):
    """op on a fresh context that holds only the state in force; a call of an accumulation: the accumulation's begin and calls so far"""
    if op.expect:
        return {"code": op.expect}                                  # a refusal's result is its code: the model gives it
    a = state.accum if op.kind in hm.ACCUM_QUERIES else None
    key = (multi, state.key() if a is None else (a.at.key(), a.begin.text(), tuple(o.text() for o in a.log)), op.but(model=0).text())
    if key in _EXPECTED:
        return _EXPECTED[key]
    c = context(multi)
    try:
        base = state if a is None else a.at
        for s_op in base.install_ops():
            assert call(c, s_op, base)["code"] == 0, s_op
        if a is not None:
            assert call(c, a.begin, base)["code"] == 0
            for o in a.log:
                if not o.expect:
                    call(c, o, base)
        out = call(c, op, base)
    finally:
        c.close()
    _EXPECTED[key] = out
    return out


def diverging(got, want):
    """-> the name of the first output that differs bit for bit, or None"""
    names = sorted(k for k in set(got) | set(want) if not k.startswith("_"))
    for k in names:
        if k not in got or k not in want:
            return k + " (missing)"
        a, b = got[k], want[k]
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                return "%s (%d of %d bytes differ)" % (k, int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1,
                                                      a.nbytes)
        elif a != b:
            return "%s (%r != %r)" % (k, a, b)
    return None


def oracle_render(O, scene_name, w, h, spp, seed):
    key = (scene_name, w, h, spp, seed)
    if key not in _ORACLE:
        t, m = hm.scene_data(scene_name)
        img, acc, scans = O.render_counter(cam_rays(w, h)[1], t, m, spp, seed)
        _ORACLE[key] = {"img": img.reshape(-1, 4), "mean": acc.reshape(-1, 3), "scans": int(scans)}
    return _ORACLE[key]


def model_render(op, state):
    """the numpy model that owns the features of op's flags, for the state's tables -> the outputs of `call`"""
    import nmap_model
    import path_model
    f = op.flags
    t, m = hm.scene_data(state.scene)
    tab = lambda bit, name: hm.table_data(name, state.scene) if f & bit else None
    est = "mis" if f & hm.MIS else "nee" if f & hm.NEE else "plain"
    args = (tab(hm.SPEC, "spec"), tab(hm.SMOOTH, "vn"), tab(hm.GLASS, "glass"), hm.env_data(state.env) if f & hm.ENV else None, tab(hm.GLOSSY, "rough"))
    if f & hm.TEX:
        m = hm.tiled_mats(state.scene)
    rays = cam_rays(op.w, op.h)[1]
    if f & hm.NMAP:
        r = nmap_model.render(rays, t, m, op.spp, op.seed, est, hm.nmap_data(), hm.table_data("uv", state.scene), *args)
    else:
        r = path_model.render(rays, t, m, op.spp, op.seed, est, *args)
    return {"img": r[0], "mean": r[1], "scans": int(r[2])}


def anchors(O, op, state, got):
    """-> (what, want) pairs from outside the library for this query's outputs"""
    if got["code"]:
        return
    names = hm.anchored_by(state, op)
    if "oracle_render" in names:
        want = oracle_render(O, state.scene, op.w, op.h, op.spp, op.seed)
        yield "the oracle's render_counter", {n: want[n] for n in want if n in got}
    if "oracle_hits" in names:
        t = hm.scene_data(state.scene)[0]
        src = source_triangles(op.w * op.h, t.shape[0]) if op.skip else None
        idx, dist = O.closest_hits(cam_rays(op.w, op.h)[1], t, src)
        yield "the oracle's closest_hits", {"idx": np.asarray(idx, np.int32), "dist": np.asarray(dist, np.float32)}
    if "oracle_total" in names:
        b = state.accum.begin
        want = oracle_render(O, state.accum.at.scene, b.w, b.h, sum(state.accum.steps()) + op.n, b.seed)
        yield "the oracle's render_counter of the total", {"img": want["img"], "mean": want["mean"]}
    if "model" in names:
        t0 = time.time()
        want = model_render(op, state)
        print("    model: %.2f s" % (time.time() - t0))
        yield "the numpy model", want


def run(program, O, multi=False):
    """the program on one context, every query compared as it goes -> None, or the failure message"""
    c = context(multi)
    state = hm.State()
    try:
        for i, op in enumerate(program):
            print("%3d  %s" % (i, op.text()))
            sys.stdout.flush()
            got = call(c, op, state)
            if "_n_launches" in got:
                print("     n_launches", got["_n_launches"])
            if op.kind in hm.SETTERS or op.kind == "accum_begin" or op.expect:
                checks = [("the status the header promises", {"code": op.expect})]
            else:
                checks = [("a fresh context", expected(op, state, multi))]
            for what, want in checks:                               # every output the call has
                bad = diverging(got, want)
                if bad:
                    return "operation %d differs from %s in %s\n%s" % (i, what, bad, hm.text(program[:i + 1]))
            for what, want in anchors(O, op, state, got):           # the outputs the outside reference has
                bad = diverging({k: got[k] for k in got if k in want}, want)
                if bad:
                    return "operation %d differs from %s in %s\n%s" % (i, what, bad, hm.text(program[:i + 1]))
            state = hm.apply(state, op)
    finally:
        c.close()
    return None


# ---------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("name", sorted(hm.HAND))
def test_hand_written_program(O, name):
    t0 = time.time()
    failure = run(hm.HAND[name], O)
    print("case time %.2f s" % (time.time() - t0))
    assert failure is None, failure


@pytest.mark.parametrize("name", sorted(hm.MULTI))
def test_hand_written_program_multi_device(O, name):
    """the host-pointer forms on Context.multi([0, 0])"""
    t0 = time.time()
    failure = run(hm.MULTI[name], O, multi=True)
    print("case time %.2f s" % (time.time() - t0))
    assert failure is None, failure


@pytest.mark.parametrize("seed", hm.SEEDS)
def test_generated_program(O, seed):
    t0 = time.time()
    failure = run(hm.program(seed, hm.LENGTH), O)
    print("case time %.2f s" % (time.time() - t0))
    assert failure is None, failure
