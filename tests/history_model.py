"""What include/spath_hip.h says is in force on a context after a sequence of calls, and programs of such calls: the model behind
tests/test_hip_history.py (a call's result does not depend on the context's history) and
tests/test_history_model.py, which holds this file to literals on the CPU.

State: the scene, the five per-triangle tables, the environment map, the atlas, the normal map, the lens and the accumulation.
Operations: small records with a one-line text form (text / parse), so that a program prints as a list that can be replayed.
Programs: program(seed, length) draws a legal one; HAND holds the hand-written ones, each named for the transition it pins.

Pure numpy and Python; the scenes and tables come from the helpers the feature tests use and are built on first use.

Not a test module."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------- flags (capi's values)
REUSE, ACCEL, NEE, MIS, CAMS = 0x100, 0x200, 0x400, 0x800, 0x1000
SPEC, SMOOTH, GLASS, ENV, GLOSSY, TEX, NMAP = 0x2000, 0x4000, 0x8000, 0x1000000, 0x2000000, 0x4000000, 0x8000000
CHUNKS_SHIFT, CHUNKS_MASK, VARIANT_MASK = 16, 0xff0000, 0xff
NEE_MIS = NEE | MIS
FEATURES = SPEC | SMOOTH | GLASS | ENV | GLOSSY | TEX | NMAP
WIDEST = NEE_MIS | SPEC | GLOSSY | GLASS | SMOOTH | ENV | TEX | NMAP
FLAG_NAMES = {"REUSE": REUSE, "ACCEL": ACCEL, "NEE": NEE, "MIS": MIS, "CAMS": CAMS, "SPEC": SPEC, "SMOOTH": SMOOTH, "GLASS": GLASS, "ENV": ENV,
              "GLOSSY": GLOSSY, "TEX": TEX, "NMAP": NMAP}
VARIANTS = (1, 2, 15, 16)                   # explicit scan variants; ACCEL is variant 8
E_INVALID, E_STATE = -1, -3


def flag_chunks(n):
    return n << CHUNKS_SHIFT


# kTableRules of spath_amd/csrc/spath_hip.hip, restated: (flag, the variants it is built for, what the context must hold, in the order
# asked, the flag it needs beside it).  variant_carried = {1, 2, 8, 15, 16}; variant_smooth = {1, 8, 16}.
CARRIED, SMOOTH_OK = (1, 2, 8, 15, 16), (1, 8, 16)
TABLE_RULES = (
    (SPEC, CARRIED, ("spec",), 0),
    (SMOOTH, SMOOTH_OK, ("vn",), 0),
    (GLASS, SMOOTH_OK, ("glass",), 0),
    (ENV, SMOOTH_OK, ("env",), 0),
    (GLOSSY, SMOOTH_OK, ("rough",), SPEC),
    (TEX, SMOOTH_OK, ("uv", "atlas"), 0),
    (NMAP, SMOOTH_OK, ("uv", "nmap"), 0),
)
TABLES = ("spec", "vn", "glass", "rough", "uv")                    # the per-triangle tables, in kTriTables' order
TABLE_SETTER = {"spec": "specular", "vn": "vertex_normals", "glass": "dielectric", "rough": "roughness", "uv": "uv"}
TABLE_FLOATS = {"spec": 4, "vn": 9, "glass": 4, "rough": 1, "uv": 6}

# ---------------------------------------------------------------------------------------------------------------- pools
SCENE_TRIS = {"hand": 3, "mirrors": 8, "clutter100": 100, "room200": 200, "room200b": 200, "dark200": 200, "room700": 700}
ENV_MAPS = {"bright8": 8, "black8": 8, "bright16": 16}
LENSES = {"pinhole": (0.0, 0.0), "wide": (0.06, 2.5)}
# pixel counts below, at and above 64, 256, 512 and 1024, and the sizes the suite already trusts
FRAMES = ((1, 1), (9, 7), (8, 8), (13, 5), (15, 17), (16, 16), (257, 1), (7, 73), (32, 16), (19, 27), (31, 33), (32, 32), (41, 25), (40, 26),
          (48, 32), (67, 41))
LARGEST = (67, 41)
RULES = ((0.3, 0.05, 4), (0.0, 0.0, 0xFFFFFFFF))                   # hip_checks.check_progressive_adaptive_denoise's rule; one that never stops a pixel
ADAPTIVE_STEPS = (4, 4, 8)
MOVES = ((0.1, -0.2, 0.3), (0.05, 0.1, 0.0))
ANCHOR = (40, 26, 3)                                              # the frame and samples of a query held to the numpy model (test_hip_history.py)
_CACHE = {}


def scene_data(name):
    """-> (tris, mats) of a pool scene.  room200b has room200's triangle count and other vertices and emitters: clutter large enough to be
    met, a smaller and tinted ceiling panel; dark200 is room200 without any emitter"""
    if ("scene", name) in _CACHE:
        return _CACHE["scene", name]
    import hip_checks as hc
    from spath_amd import scene
    F = np.float32
    if name == "hand":
        t, m = hc.hand_scene()[:2]
    elif name == "mirrors":
        t, m = hc.facing_mirrors()[:2]
    elif name == "clutter100":
        t, m = scene.open_clutter(100)
    elif name in ("room200", "room700"):
        t, m = scene.closed_room(int(name[4:]))
    elif name == "dark200":
        t, m = scene.closed_room(200)
        m = m.copy()
        m[:, 3:6] = 0
    elif name == "room200b":
        t, m = scene.closed_room(200, seed=0xB0B, clutter_scale=8.0)
        t, m = t.copy(), m.copy()
        for v in range(3):
            t[12:14, 3 * v] *= F(0.5)
            t[12:14, 3 * v + 2] *= F(0.5)
        t = scene.flat_normals(t)
        m[12:14, 3:6] = (2.0, 1.0, 0.5)
        m[20:60:4, 3:6] = (0.0, 0.5, 1.0)
    else:
        raise KeyError(name)
    _CACHE["scene", name] = (np.ascontiguousarray(t, F), np.ascontiguousarray(m, F))
    return _CACHE["scene", name]


def table_data(table, scene_name, bad=False):
    """the table of a pool scene, by the helpers of the feature tests; bad: one row (n // 2) that the setter's rule refuses"""
    key = ("table", table, scene_name, bad)
    if key in _CACHE:
        return _CACHE[key]
    import hip_checks as hc
    from spath_amd import scene
    F = np.float32
    t, m = scene_data(scene_name)
    n = t.shape[0]
    if table == "spec":
        x = hc.mixed_table(t, m)
    elif table == "vn":
        x = scene.vertex_normals(t)
    elif table == "glass":
        i = np.arange(n)
        x = scene.dielectric_table(t, 1.5, (0.9, 0.95, 1.0), which=i[(i % 5 == 3) & (m[:, 3:6].sum(1) == 0)])
    elif table == "rough":
        x = np.array([0, 0.05, 0.3, 1], F)[np.random.default_rng(5).integers(0, 4, n)]
    elif table == "uv":
        from test_hip_texture import tile_uv
        x = tile_uv(n)
    else:
        raise KeyError(table)
    x = np.ascontiguousarray(x, F).reshape(n, TABLE_FLOATS[table]).copy()
    if bad:
        x[n // 2, -1] = {"spec": 1.5, "vn": np.nan, "glass": 0.5, "rough": 1.5, "uv": np.nan}[table]
    _CACHE[key] = x
    return x


def env_data(name, bad=False):
    from spath_amd import scene
    n = ENV_MAPS[name]
    x = np.zeros((n, n, 3), np.float32) if name.startswith("black") else np.ascontiguousarray(scene.sky_environment(n), np.float32).copy()
    if bad:
        x[n // 2, 1, 2] = -1.0
    return x


def atlas_data(bad=False):
    from test_hip_texture import TILE_ATLAS
    x = np.ascontiguousarray(TILE_ATLAS, np.float32).copy()
    if bad:
        x[3, 2, 1] = np.nan
    return x


def nmap_data():
    from test_hip_normal_map import TILE_MAP
    return np.ascontiguousarray(TILE_MAP, np.float32)


def tiled_mats(scene_name):
    """the materials whose untextured render equals the textured one under table_data("uv") and atlas_data(): triangle i sees tile i % 6
    alone (tests/test_hip_texture.py: the tile equivalence)"""
    from test_hip_texture import TILE_COLOURS
    m = scene_data(scene_name)[1]
    m2 = m.copy()
    m2[:, :3] = (m[:, :3] * TILE_COLOURS[np.arange(m.shape[0]) % 6]).astype(np.float32)
    return m2


# ---------------------------------------------------------------------------------------------------------------- operations
# kind -> its fields in text order.  "expect" (the code of a marked refusal), "bad" (a setter's refused input) and "model" (a render that
# the test also holds to the numpy model) are optional and come last
FIELDS = {
    "set_scene": ("name", "form", "stream"),
    "set_table": ("table", "form", "stream"),
    "set_env": ("map", "form", "stream"),
    "set_atlas": ("form", "stream"),
    "set_nmap": ("form", "stream"),
    "set_lens": ("lens",),
    "render": ("w", "h", "spp", "seed", "mode", "flags"),
    "render_camera": ("w", "h", "spp", "seed", "flags"),
    "render_device": ("w", "h", "spp", "seed", "mode", "flags", "accum", "stream"),
    "render_device_accum": ("w", "h", "spp", "split", "seed", "flags", "stream"),
    "closest_hit_device": ("w", "h", "flags", "skip", "stream"),
    "accum_begin": ("w", "h", "seed", "flags", "src", "rule"),
    "accum_step": ("n",),
    "accum_counts": (),
    "accum_gbuffer": (),
    "accum_denoise": (),
    "gbuffer_device": ("w", "h", "flags", "stream"),
    "denoise_device": ("w", "h", "var", "stream"),
}
OPTIONAL = ("bad", "model", "expect")
SETTERS = ("set_scene", "set_table", "set_env", "set_atlas", "set_nmap", "set_lens")
ACCUM_QUERIES = ("accum_step", "accum_counts", "accum_gbuffer", "accum_denoise")
STRING_FIELDS = ("name", "form", "table", "map", "lens", "mode", "src")


class Op:
    """one call: its kind and its arguments.  Two ops are equal when their text is"""
    __slots__ = ("kind", "a")

    def __init__(self, kind, **a):
        want = FIELDS[kind]
        assert tuple(k for k in a if k not in OPTIONAL) == want, (kind, tuple(a), want)
        self.kind, self.a = kind, dict(a)

    def __getattr__(self, k):
        try:
            return self.a[k]
        except KeyError:
            if k in OPTIONAL:
                return 0
            raise AttributeError(k)

    def text(self):
        def show(k, v):
            return "%s=%s" % (k, "0x%x" % v if k == "flags" else v)
        words = [show(k, self.a[k]) for k in FIELDS[self.kind]] + [show(k, self.a[k]) for k in OPTIONAL if self.a.get(k, 0)]
        return " ".join([self.kind] + words)

    def __eq__(self, other):
        return isinstance(other, Op) and self.text() == other.text()

    def __hash__(self):
        return hash(self.text())

    def __repr__(self):
        return self.text()

    def but(self, **a):
        """this op with some arguments replaced (or, with 0, dropped, for the optional ones)"""
        b = dict(self.a)
        b.update(a)
        return Op(self.kind, **{k: v for k, v in b.items() if k not in OPTIONAL or v})


def parse_op(line):
    words = line.split()
    a = {}
    for word in words[1:]:
        k, v = word.split("=", 1)
        a[k] = v if k in STRING_FIELDS else int(v, 0)
    return Op(words[0], **a)


def text(program):
    return "\n".join(op.text() for op in program)


def parse(s):
    return [parse_op(line) for line in s.split("\n") if line.strip()]


# ---------------------------------------------------------------------------------------------------------------- the flag rules
def resolved_variant(flags, n_tris):
    """pick_variant: SPHIP_FLAG_ACCEL is 8, then the low byte, then 1 below 64 triangles and 16 from there"""
    if flags & ACCEL:
        return 8
    v = flags & VARIANT_MASK
    if v:
        return v
    return 1 if n_tris < 64 else 16


def check_flags(state, flags, pt=True, have_cam=False):
    """what a path-traced (or, pt False, a flat) render of the state answers to `flags`: 0, E_INVALID or E_STATE, in check_render's order:
    MIS without NEE, the camera rule, then the table rules as listed, each one: flat mode, NEE alone, the variant, the companion flag
    (E_INVALID) and only then the table (E_STATE)"""
    v = resolved_variant(flags, SCENE_TRIS[state.scene])
    if v not in CARRIED:
        return E_INVALID
    if pt and flags & MIS and not flags & NEE:
        return E_INVALID
    if pt and flags & CAMS:
        if not have_cam or flags & REUSE:
            return E_INVALID
    for bit, variants, needs, with_ in TABLE_RULES:
        if not flags & bit:
            continue
        if not pt:
            return E_INVALID
        if flags & NEE and not flags & MIS:
            return E_INVALID
        if v not in variants:
            return E_INVALID
        if with_ and not flags & with_:
            return E_INVALID
        for need in needs:
            if not state.has(need):
                return E_STATE
    return 0


# ---------------------------------------------------------------------------------------------------------------- the state
class Accum:
    """an accumulation: the op that began it, the state it was begun in, every accum_* call since, and whether a setter has ended it"""
    def __init__(self, begin, at):
        self.begin, self.at, self.log, self.ended = begin, at, [], False

    def steps(self):
        return [op.n for op in self.log if op.kind == "accum_step" and not op.expect]

    def copy(self):
        c = Accum(self.begin, self.at)
        c.log, c.ended = list(self.log), self.ended
        return c


class State:
    """what the header says is in force.  key() names everything a stateless query may depend on"""
    def __init__(self):
        self.scene = None
        self.tables = {t: False for t in TABLES}
        self.env = None
        self.atlas = self.nmap = False
        self.lens = "pinhole"
        self.accum = None

    def copy(self):
        s = State()
        s.scene, s.tables, s.env, s.atlas, s.nmap, s.lens = self.scene, dict(self.tables), self.env, self.atlas, self.nmap, self.lens
        s.accum = self.accum.copy() if self.accum else None
        return s

    def has(self, what):
        return bool(self.tables[what]) if what in TABLES else bool(getattr(self, what))

    def key(self):
        return (self.scene, tuple(t for t in TABLES if self.tables[t]), self.env, self.atlas, self.nmap, self.lens)

    def install_ops(self):
        """the setters that bring a fresh context to this state (host forms), in an order of their own: the context-level items first,
        which need no scene"""
        ops = [Op("set_lens", lens=self.lens)]
        if self.env:
            ops.append(Op("set_env", map=self.env, form="host", stream=0))
        if self.atlas:
            ops.append(Op("set_atlas", form="host", stream=0))
        if self.nmap:
            ops.append(Op("set_nmap", form="host", stream=0))
        if self.scene:
            ops.append(Op("set_scene", name=self.scene, form="host", stream=0))
            ops += [Op("set_table", table=t, form="host", stream=0) for t in TABLES if self.tables[t]]
        return ops


def expected_code(state, op):
    """the status the header promises for op in state: 0, E_INVALID or E_STATE"""
    k = op.kind
    if k == "set_table":
        # "SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite ..." (sphip_set_specular and its four siblings)
        return E_STATE if state.scene is None else E_INVALID if op.bad else 0
    if k in SETTERS:
        return E_INVALID if op.bad else 0
    if k in ("render", "render_camera", "render_device", "render_device_accum"):
        if state.scene is None:
            return E_STATE
        return check_flags(state, op.flags, pt=k in ("render_camera", "render_device_accum") or op.mode == "pt", have_cam=k == "render_camera")
    if k in ("closest_hit_device", "denoise_device"):
        return E_STATE if state.scene is None else 0
    if k == "gbuffer_device":
        # sphip_gbuffer_device: "with the flag and normals set ..." -- the flag without them is the table rule's E_STATE
        if state.scene is None or (op.flags & SMOOTH and not state.has("vn")) or (op.flags & NMAP and not (state.has("uv") and state.has("nmap"))):
            return E_STATE
        return 0
    if k == "accum_begin":
        if state.scene is None:
            return E_STATE
        return check_flags(state, op.flags, pt=True, have_cam=op.src == "cam")
    a = state.accum
    if k == "accum_counts":
        return E_STATE if a is None else 0                       # "SPHIP_E_STATE when no accumulation has been begun"
    if k == "accum_step":
        # "SPHIP_E_STATE when no accumulation was begun or a scene has been set since the begin"
        return E_STATE if a is None or a.ended else 0
    if k == "accum_gbuffer":
        return E_STATE if a is None or a.ended else 0            # "SPHIP_E_STATE with no accumulation or after a set_scene since the begin"
    if k == "accum_denoise":
        return E_STATE if a is None or a.ended or not a.steps() else 0   # "SPHIP_E_STATE before the first step or after a set_scene since the begin"
    raise KeyError(k)


def apply(state, op):
    """-> the state after op.  The transition rules, each with the sentence of include/spath_hip.h it restates"""
    s = state.copy()
    code = expected_code(state, op)
    k = op.kind
    if k in SETTERS and code != 0:
        # "(the message names the first such triangle; the table stays as it was)": a refused setter changes nothing, the accumulation included
        return s
    if k == "set_scene":
        # "Every set_scene clears the table." (each per-triangle table's setter)
        s.scene, s.tables = op.name, {t: False for t in TABLES}
        # "Unlike the per-triangle tables the map is NOT cleared by sphip_set_scene"; atlas and normal map: "kept across set_scene and needs
        # no scene"; the lens is the context's ("for its later camera-sample renders"): all four stay
        # sphip_accum_step: "SPHIP_E_STATE when ... a scene has been set since the begin"
        if s.accum:
            s.accum.ended = True
    elif k in ("set_table", "set_env", "set_atlas", "set_nmap"):
        # "During an accumulation it ends the accumulation as a set_scene does (the next step: SPHIP_E_STATE)."
        if k == "set_table":
            s.tables[op.table] = True
        elif k == "set_env":
            s.env = op.map
        elif k == "set_atlas":
            s.atlas = True
        else:
            s.nmap = True
        if s.accum:
            s.accum.ended = True
    elif k == "set_lens":
        # "An accumulation captures the lens at its begin: a later sphip_set_lens applies from the next begin."
        s.lens = op.lens
    elif k == "accum_begin":
        # a begin replaces the accumulation; one that is refused after its argument checks "leaves no accumulation behind"
        s.accum = Accum(op, state.copy()) if code == 0 else None
        if s.accum:
            s.accum.at.accum = None
    elif k in ACCUM_QUERIES:
        # "sphip_render / sphip_render_camera calls in between do not disturb it": only the accumulation's own calls move it on
        if s.accum:
            s.accum.log.append(op)
    return s


def anchored_by(state, op):
    """the references outside the library that a query in `state` is also held to (tests/test_hip_history.py): "oracle_render" for a
    path-traced render with no flag but a variant, sample chunks or primary-hit reuse; "oracle_hits" for a hit query outside the BVH;
    "oracle_total" for a step of a plain accumulation with such flags; "model" for the render marked for the numpy model"""
    if op.expect:
        return []
    k, other = op.kind, FEATURES | NEE | MIS | CAMS | ACCEL
    names = []
    if k in ("render", "render_camera", "render_device") and op.a.get("mode", "pt") == "pt" and not op.flags & other:
        names.append("oracle_render")
    if k == "closest_hit_device" and not op.flags & ACCEL:
        names.append("oracle_hits")
    a = state.accum
    if k == "accum_step" and a and not a.ended and a.begin.rule < 0 and not a.begin.flags & other:
        names.append("oracle_total")
    if op.model:
        names.append("model")
    return names


def run_model(program, state=None):
    """-> the states before each op, and the final one"""
    state = state or State()
    states = []
    for op in program:
        states.append(state)
        state = apply(state, op)
    return states, state


def legal(program):
    """every op carries the code the rules give it"""
    states, _ = run_model(program)
    return all(op.expect == expected_code(s, op) for s, op in zip(states, program))


# ---------------------------------------------------------------------------------------------------------------- the launch plan, restated
# sp_host_plan.h: what the two-stage path-tracing kernels park per work slot in `work`
SLOT_HIST, SLOT_ACC, SLOT_NEE_L, SLOT_MIS_D = 40, 12, 48, 60
TWO_STAGE = {15: (4, True), 16: (1, False)}          # variant -> (R, split)
CHUNK_TARGET_BLOCKS = 262144


def work_need(state, op):
    """-> (bytes of `work` a path-traced launch needs, its slot size) by plan_launch's arithmetic, (0, 0) for a launch that parks nothing
    there.  The default scan's workgroup is taken as 256 threads, the device's free memory as ample, and an adaptive step as the whole
    frame: the figure serves the coverage counts of tests/test_history_model.py, not a comparison"""
    k = op.kind
    if k == "accum_step":
        if not state.accum or state.accum.ended:
            return 0, 0
        b = state.accum.begin
        w, h, spp, flags, n_tris = b.w, b.h, op.n, b.flags, SCENE_TRIS[state.accum.at.scene]
    elif k in ("render", "render_camera", "render_device", "render_device_accum"):
        if op.expect or state.scene is None or (k in ("render", "render_device") and op.mode != "pt"):
            return 0, 0
        w, h, spp, flags, n_tris = op.w, op.h, op.spp, op.flags, SCENE_TRIS[state.scene]
    else:
        return 0, 0
    v = resolved_variant(flags, n_tris)
    if v not in TWO_STAGE:
        return 0, 0
    R, split = TWO_STAGE[v]
    n_rays = w * h
    slots = R if split else 1
    rays_per_block = 256 if split else 256 * R
    lanes = (n_rays + 1023) // 1024 * 1024 * slots
    px_blocks = (n_rays + rays_per_block - 1) // rays_per_block
    n_iter = (spp + slots - 1) // slots
    forced = (flags & CHUNKS_MASK) >> CHUNKS_SHIFT
    chunks = forced or 1
    while not forced and px_blocks * chunks < CHUNK_TARGET_BLOCKS and chunks < 128:
        chunks *= 2
    chunks = min(chunks, n_iter)
    slot = SLOT_HIST + SLOT_ACC + (SLOT_MIS_D if flags & MIS else SLOT_NEE_L if flags & NEE else 0)
    return lanes * chunks * slot, slot


def coverage(program):
    """-> dict of counts over one program: ensure() reuses of `work` (a launch that needs fewer bytes than the running maximum, so it runs
    in a buffer that holds another launch's bytes), pack changes on a reused buffer (such a launch whose slot size or slot count differs
    from the launch before it: the regions lie at other offsets), and set_scene transitions to more and to fewer triangles"""
    states, _ = run_model(program)
    c = {"reuses": 0, "pack_changes": 0, "grow": 0, "shrink": 0}
    cap, last = 0, None
    for s, op in zip(states, program):
        if op.kind == "set_scene" and s.scene is not None:
            d = SCENE_TRIS[op.name] - SCENE_TRIS[s.scene]
            c["grow"] += d > 0
            c["shrink"] += d < 0
        need = work_need(s, op)
        if not need[0]:
            continue
        if need[0] < cap:
            c["reuses"] += 1
            c["pack_changes"] += last is not None and need != last
        cap, last = max(cap, need[0]), need
    return c


# ---------------------------------------------------------------------------------------------------------------- programs
def _all_tables(form="host"):
    return [Op("set_table", table=t, form=form, stream=i % 2) for i, t in enumerate(TABLES)]


def _context_items(env="bright16"):
    return [Op("set_env", map=env, form="host", stream=0), Op("set_atlas", form="host", stream=0), Op("set_nmap", form="host", stream=0)]


def warm_up():
    """every scratch buffer large and full of another launch's bytes: the largest frame at 16 spp under the widest legal pack, an adaptive
    accumulation of three steps, a denoise"""
    return ([Op("set_scene", name="room700", form="host", stream=0)] + _all_tables() + _context_items() + [Op("set_lens", lens="wide")] +
            [Op("render", w=LARGEST[0], h=LARGEST[1], spp=16, seed=2, mode="pt", flags=WIDEST),
             Op("accum_begin", w=48, h=32, seed=9, flags=WIDEST, src="rays", rule=0)] +
            [Op("accum_step", n=n) for n in ADAPTIVE_STEPS] + [Op("accum_denoise")])


PACKS = {"plain": 0, "nee": NEE, "mis": NEE_MIS, "env": NEE_MIS | ENV, "tex": NEE_MIS | ENV | TEX, "nmap": NEE_MIS | ENV | TEX | NMAP, "widest": WIDEST}


def _model_render(flags, seed=3):
    w, h, spp = ANCHOR
    return Op("render", w=w, h=h, spp=spp, seed=seed, mode="pt", flags=flags, model=1)


def order_of_5_17(pack):
    """DESIGN.md section 5.17's order: an adaptive accumulation over 48 x 32 in steps 4, 4, 8, a 40 x 26 camera render with the same flags,
    one more step, the camera render again"""
    f = PACKS[pack]
    cam = Op("render_camera", w=40, h=26, spp=4, seed=6, flags=f)
    return ([Op("set_scene", name="clutter100", form="host", stream=0)] + _all_tables() + _context_items("bright8") +
            [Op("accum_begin", w=48, h=32, seed=9, flags=f, src="rays", rule=0)] + [Op("accum_step", n=n) for n in ADAPTIVE_STEPS] +
            [cam, Op("accum_step", n=4), Op("accum_counts"), cam, _model_render(f)] +
            # and a plain accumulation over the camera's frame in the buffers the adaptive one leaves: with no flags its steps have the oracle
            [Op("accum_begin", w=40, h=26, seed=9, flags=f, src="cam", rule=-1), Op("accum_step", n=3), Op("accum_step", n=5)])


def large_small_large(pack, other):
    """67 x 41 at 16 spp, 1 x 1 at 1 spp, 9 x 7 at 3 spp, 67 x 41 at 2 spp for the two-stage variants, then the small calls under another
    pack: `work` is read with other offsets"""
    f, g = PACKS[pack], PACKS[other]
    ops = [Op("set_scene", name="room200", form="host", stream=0)] + _all_tables() + _context_items("bright8")
    for v in (16,) if f & FEATURES & ~SPEC else (15, 16):
        for w, h, spp in ((67, 41, 16), (1, 1, 1), (9, 7, 3), (67, 41, 2)):
            ops.append(Op("render", w=w, h=h, spp=spp, seed=5, mode="pt", flags=f | v))
        for w, h, spp in ((1, 1, 1), (9, 7, 3)):
            ops.append(Op("render", w=w, h=h, spp=spp, seed=5, mode="pt", flags=g | (16 if g & FEATURES & ~SPEC else v)))
    # a small plain accumulation with no flag but the variant, in the buffers the large calls leave: its steps have the oracle
    ops += [Op("accum_begin", w=9, h=7, seed=5, flags=16, src="rays", rule=-1), Op("accum_step", n=3), Op("accum_step", n=2)]
    return ops + [_model_render(f | 16)]


def scene_change_with_tables():
    """all tables and a render; a smaller scene: every per-triangle flag is refused while the map, the atlas, the normal map and the lens
    still work; the tables again; a larger scene; the zero stand-ins follow n_tris both ways (DIELECTRIC alone, NORMAL_MAP without SMOOTH)"""
    wide = Op("render", w=19, h=27, spp=3, seed=4, mode="pt", flags=WIDEST)
    alone = [Op("render", w=13, h=5, spp=2, seed=4, mode="pt", flags=NEE_MIS | GLASS), Op("render", w=13, h=5, spp=2, seed=4, mode="pt", flags=NMAP),
             Op("render", w=13, h=5, spp=2, seed=4, mode="pt", flags=NEE_MIS | ENV)]
    ops = [Op("set_scene", name="room200", form="host", stream=0)] + _all_tables() + _context_items("bright8") + [Op("set_lens", lens="wide"), wide] + alone
    for name in ("clutter100", "room700"):
        ops.append(Op("set_scene", name=name, form="host", stream=0))
        ops += [Op("render", w=13, h=5, spp=2, seed=4, mode="pt", flags=f, expect=E_STATE) for f in (SPEC, SMOOTH, GLASS, SPEC | GLOSSY, TEX, NMAP)]
        ops += [Op("render", w=13, h=5, spp=2, seed=4, mode="pt", flags=NEE_MIS | ENV),
                Op("render_camera", w=13, h=5, spp=2, seed=4, flags=CAMS)]
        ops += _all_tables() + [wide] + alone
    return ops + [_model_render(NEE_MIS | GLASS | SPEC)]


def same_size_swap():
    """FLAG_ACCEL, variant 15 and variant 16 under NEE|MIS, the same-count scene with other vertices and emitters, the three again: a stale
    record stream, BVH or light table changes an image there"""
    three = [Op("render", w=40, h=26, spp=3, seed=7, mode="pt", flags=NEE_MIS | v) for v in (ACCEL, 15, 16)]
    hits = [Op("closest_hit_device", w=40, h=26, flags=v, skip=0, stream=i % 2) for i, v in enumerate((ACCEL, 15, 16))]
    return ([Op("set_scene", name="room200", form="host", stream=0)] + three + hits + [Op("set_scene", name="room200b", form="host", stream=0)] +
            three + hits + [_model_render(NEE_MIS | 16)])


def environment_transitions():
    """under NEE|MIS|ENVIRONMENT: a bright map, a black one, a bright one of another size, then set_scene (the map is kept, its
    scene-dependent part rebuilt), then a scene with no emitter at all"""
    r = Op("render", w=32, h=16, spp=3, seed=8, mode="pt", flags=NEE_MIS | ENV)
    ops = [Op("set_scene", name="clutter100", form="host", stream=0)]
    for i, mp in enumerate(("bright8", "black8", "bright16")):
        ops += [Op("set_env", map=mp, form="device" if i == 1 else "host", stream=1), r]
    ops += [Op("set_scene", name="room200", form="host", stream=0), r, Op("set_scene", name="dark200", form="host", stream=0), r,
            Op("set_env", map="black8", form="host", stream=0), r, Op("set_env", map="bright8", form="host", stream=0), r,
            Op("set_scene", name="clutter100", form="device", stream=1), _model_render(NEE_MIS | ENV)]
    return ops


def denoiser_state():
    """an adaptive accumulation, a step, a denoise, set_scene (the material classes are rebuilt), again; gbuffer_device and
    denoise_device on another frame size in between"""
    ops = []
    for name in ("room200", "clutter100"):
        ops += [Op("set_scene", name=name, form="host", stream=0), Op("accum_begin", w=32, h=32, seed=3, flags=NEE_MIS, src="cam", rule=0),
                Op("accum_step", n=4), Op("accum_denoise"), Op("gbuffer_device", w=19, h=27, flags=0, stream=0),
                Op("denoise_device", w=19, h=27, var=1, stream=1), Op("accum_step", n=4), Op("accum_gbuffer"), Op("accum_denoise")]
    return ops + [_model_render(NEE_MIS)]


def refusals_change_nothing():
    """every refused setter and query, each followed by the query that preceded it"""
    q = Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=WIDEST)
    ops = [Op("set_table", table=t, form="host", stream=0, expect=E_STATE) for t in TABLES]              # before any scene
    ops += [Op("set_scene", name="room200", form="host", stream=0)] + _all_tables() + _context_items("bright8") + [q]
    for t in TABLES:
        ops += [Op("set_table", table=t, form="host", stream=0, bad=1, expect=E_INVALID), q]
    ops += [Op("set_env", map="bright8", form="host", stream=0, bad=1, expect=E_INVALID), q,
            Op("set_atlas", form="host", stream=0, bad=1, expect=E_INVALID), q,
            Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=MIS, expect=E_INVALID), q,
            Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=NEE | SPEC, expect=E_INVALID), q,
            Op("render", w=15, h=17, spp=2, seed=5, mode="flat", flags=SPEC, expect=E_INVALID), q,
            Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=SMOOTH | 15, expect=E_INVALID), q]
    # an accumulation that a refused setter leaves alone, then one that a setter ends: the step after it is refused, the render is not
    ops += [Op("accum_begin", w=16, h=16, seed=3, flags=NEE_MIS | SPEC, src="rays", rule=-1), Op("accum_step", n=2),
            Op("set_table", table="spec", form="host", stream=0, bad=1, expect=E_INVALID), Op("accum_step", n=3),
            Op("set_table", table="rough", form="host", stream=0), Op("accum_step", n=1, expect=E_STATE), Op("accum_counts"),
            Op("accum_denoise", expect=E_STATE), q]
    ops += [Op("set_scene", name="clutter100", form="host", stream=0), Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=SPEC, expect=E_STATE),
            Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=NEE_MIS | ENV | NMAP, expect=E_STATE),
            Op("render", w=15, h=17, spp=2, seed=5, mode="pt", flags=NEE_MIS | ENV), _model_render(NEE_MIS | ENV)]
    return ops


HAND = {}
for _p in PACKS:
    HAND["order_of_5_17[%s]" % _p] = order_of_5_17(_p)
HAND["large_small_large[mis]"] = large_small_large("mis", "tex")
HAND["large_small_large[tex]"] = large_small_large("tex", "plain")
HAND["scene_change_with_tables"] = scene_change_with_tables()
HAND["same_size_swap"] = same_size_swap()
HAND["environment_transitions"] = environment_transitions()
HAND["denoiser_state"] = denoiser_state()
HAND["refusals_change_nothing"] = refusals_change_nothing()
# the host-pointer calls alone, as a multi-device context takes them
MULTI = {"order_of_5_17[plain]": HAND["order_of_5_17[plain]"], "order_of_5_17[mis]": HAND["order_of_5_17[mis]"],
         "scene_change_with_tables": HAND["scene_change_with_tables"]}


# ---------------------------------------------------------------------------------------------------------------- the generator
def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def draw_flags(rng, state, cam=False):
    """a flag word that check_flags accepts for a path-traced render of the state; one in five is bare (a variant, sample chunks or
    primary-hit reuse at the most), the renders that the oracle itself can check"""
    if rng.random() < 0.2:
        return (_pick(rng, (0, 1, 2, 15, 16)) | _pick(rng, (0, 0, flag_chunks(1), flag_chunks(4))) | (REUSE if rng.random() < 0.3 else 0))
    est = _pick(rng, (0, NEE_MIS, NEE_MIS, NEE))
    f = est
    if est != NEE:
        for bit, _, needs, with_ in TABLE_RULES:
            if all(state.has(n) for n in needs) and (not with_ or f & with_) and rng.random() < 0.5:
                f |= bit
    narrow = bool(f & FEATURES & ~SPEC)
    f |= _pick(rng, (0, 1, 16, ACCEL) if narrow else (0, 1, 2, 15, 16, ACCEL))
    r = rng.random()
    if r < 0.15:
        f |= 1 << CHUNKS_SHIFT
    elif r < 0.3:
        f |= 4 << CHUNKS_SHIFT
    if cam and rng.random() < 0.5:
        f |= CAMS
    elif rng.random() < 0.2:
        f |= REUSE
    assert check_flags(state, f, True, cam) == 0, hex(f)
    return f


def draw_scan_flags(rng):
    """flat renders and hit queries ignore the feature flags: a variant, with or without primary-hit reuse"""
    return _pick(rng, (0, 1, 2, 15, 16, ACCEL)) | (REUSE if rng.random() < 0.2 else 0)


def _draw_setter(rng, state):
    form, stream = _pick(rng, ("host", "device")), int(rng.integers(0, 2))
    r = rng.random()
    if r < 0.55:
        return Op("set_table", table=_pick(rng, TABLES), form=form, stream=stream)
    if r < 0.7:
        return Op("set_env", map=_pick(rng, tuple(ENV_MAPS)), form=form, stream=stream)
    if r < 0.8:
        return Op("set_atlas", form=form, stream=stream)
    if r < 0.9:
        return Op("set_nmap", form=form, stream=stream)
    return Op("set_lens", lens=_pick(rng, tuple(LENSES)))


def _draw_refusal(rng, state):
    w, h = _pick(rng, FRAMES[:8])
    missing = [bit for bit, _, needs, with_ in TABLE_RULES if not all(state.has(n) for n in needs) and bit != GLOSSY]
    r = rng.random()
    if r < 0.3:
        op = Op("set_table", table=_pick(rng, TABLES), form="host", stream=0, bad=1)
    elif r < 0.4:
        op = Op("set_env", map="bright8", form="host", stream=0, bad=1)
    elif r < 0.6 or not missing:
        op = Op("render", w=w, h=h, spp=2, seed=5, mode="pt", flags=MIS | draw_scan_flags(rng))
    else:
        op = Op("render", w=w, h=h, spp=2, seed=5, mode="pt", flags=_pick(rng, missing) | _pick(rng, (0, NEE_MIS)))
    return op.but(expect=expected_code(state, op))


def _draw_query(rng, state, spp):
    w, h = _pick(rng, FRAMES)
    seed, stream = int(rng.integers(1, 9)), int(rng.integers(0, 2))
    a = state.accum
    live = a is not None and not a.ended
    kinds = ["render", "render", "render_flat", "render_camera", "render_device", "render_device_accum", "closest_hit_device", "accum_begin",
             "gbuffer_device", "denoise_device"]
    if live:
        kinds += ["accum_step"] * 4 + ["accum_counts", "accum_gbuffer"] + (["accum_denoise"] * 2 if a.steps() else [])
    elif a is not None:
        kinds += ["accum_step_ended"]
    k = _pick(rng, kinds)
    if k == "render":
        return Op("render", w=w, h=h, spp=spp, seed=seed, mode="pt", flags=draw_flags(rng, state))
    if k == "render_flat":
        return Op("render", w=w, h=h, spp=1, seed=seed, mode="flat", flags=draw_scan_flags(rng))
    if k == "render_camera":
        return Op("render_camera", w=w, h=h, spp=spp, seed=seed, flags=draw_flags(rng, state, cam=True))
    if k == "render_device":
        pt = rng.random() < 0.7
        return Op("render_device", w=w, h=h, spp=spp if pt else 1, seed=seed, mode="pt" if pt else "flat",
                  flags=draw_flags(rng, state) if pt else draw_scan_flags(rng), accum=int(rng.integers(0, 2)), stream=stream)
    if k == "render_device_accum":
        n = max(spp, 2)
        return Op("render_device_accum", w=w, h=h, spp=n, split=int(rng.integers(1, n)), seed=seed, flags=draw_flags(rng, state), stream=stream)
    if k == "closest_hit_device":
        return Op("closest_hit_device", w=w, h=h, flags=draw_scan_flags(rng), skip=int(rng.integers(0, 2)), stream=stream)
    if k == "accum_begin":
        cam = rng.random() < 0.5
        return Op("accum_begin", w=w, h=h, seed=seed, flags=draw_flags(rng, state, cam=cam), src="cam" if cam else "rays", rule=int(rng.integers(-1, 2)))
    if k == "gbuffer_device":
        f = draw_scan_flags(rng)
        if f & VARIANT_MASK in (0, 1, 16):
            f |= (SMOOTH if state.has("vn") and rng.random() < 0.5 else 0) | (NMAP if state.has("uv") and state.has("nmap") and rng.random() < 0.5 else 0)
        return Op("gbuffer_device", w=w, h=h, flags=f, stream=stream)
    if k == "denoise_device":
        return Op("denoise_device", w=w, h=h, var=int(rng.integers(0, 2)), stream=stream)
    if k == "accum_step":
        return Op("accum_step", n=_pick(rng, (1, 2, 3, 4, 5, 8)))
    if k == "accum_step_ended":
        return Op("accum_step", n=2, expect=E_STATE)
    return Op(k)


def program(seed, length=40):
    """a legal program drawn from numpy's generator: the warm-up, then scene changes, setters, marked refusals and queries.  Samples per
    pixel are 1 to 5, and 16 once (the "large" call)"""
    rng = np.random.default_rng(seed)
    ops = warm_up()
    state = run_model(ops)[1]
    large_at = len(ops) + int(rng.integers(3, max(4, length - len(ops))))
    while len(ops) < length:
        r = rng.random()
        if r < 0.12:
            op = Op("set_scene", name=_pick(rng, tuple(SCENE_TRIS)), form=_pick(rng, ("host", "device")), stream=int(rng.integers(0, 2)))
        elif r < 0.32:
            op = _draw_setter(rng, state)
        elif r < 0.40:
            op = _draw_refusal(rng, state)
        else:
            op = _draw_query(rng, state, 16 if len(ops) >= large_at else int(rng.integers(1, 6)))
            if op.a.get("spp") == 16:
                large_at = 1 << 30
        assert op.expect == expected_code(state, op), op
        ops.append(op)
        state = apply(state, op)
    return ops


# chosen on the CPU (tests/test_history_model.py asserts what they cover)
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
LENGTH = 40
