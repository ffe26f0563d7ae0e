"""What the scene entry points refuse, and in which order.  One entry point of each family whose validators share code in
hfcl_host_scene.hip -- nearest, nearest_self, nearest_env, self_pairs and env_pairs (host and device), the narrow phase on a list of pairs
(collide_pairs_device, collide_env_pairs_device), collide_self, collide_env -- with every refusal it has: the return code and the whole
text of hfcl_last_error().  The other scene suites pin a word of single refusals; here the texts are whole and, for every two refusals of
a family that can apply to one call, the one that stands earlier in the family's list below wins.

The codes, the texts and the order of a family's list were recorded from the library as it stood before the validators were merged (the
whole table, and every combinable two, were run against it first); a change of a text or of the precedence is a change of the C ABI's
behaviour and shows here.

The scene: six solids, all 15 pairs, 2 configurations; for the env families the first four move.  Nothing here computes more than a list
of at most 30 pairs."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_OBJ, N_CONF, N_MOVING = 6, 2, 4
NAN = float("nan")

# scene handles a case can ask for instead of the family's own
NULL, STALE, NO_ENV, ENV32 = "null scene", "stale scene", "no environment", "environment of the other precision"


class Ctx:
    pass


def make_ctx(pkg, torch):
    abi, d = pkg.abi, pkg.engine.dll()
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    obj_shape = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint32)
    rng = np.random.default_rng(23)
    quat = pkg.workloads.uniform_quaternions(rng, N_CONF * N_OBJ)
    T = rng.uniform(-1, 1, (N_CONF * N_OBJ, 3))
    c = Ctx()
    c.table = np.ascontiguousarray(pkg.geometry.make_pose(quat=quat, T=T).reshape(N_CONF, N_OBJ, 12))
    pose = np.ascontiguousarray(pkg.geometry.pose_f32_from_quat(quat, T).reshape(N_CONF, N_OBJ, 7))
    i, j = np.triu_indices(N_OBJ, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    c.lib = pkg.Library(L)
    c.plain = c.lib.scene(obj_shape, pairs)
    c.env = c.lib.scene(obj_shape, pairs)
    c.env.set_environment(N_MOVING, c.table[0, N_MOVING:])
    c.env32 = c.lib.scene(obj_shape, pairs)
    c.env32.set_environment(N_MOVING, pose[0, N_MOVING:])
    # a scene whose library's shapes were replaced after it was made
    c.lib2 = pkg.Library(L)
    c.stale = c.lib2.scene(obj_shape, pairs)
    shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
    assert d.hfcl_lib_set_shapes(c.lib2._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
    c.moving = np.ascontiguousarray(c.table[:, :N_MOVING])
    c.d_table = torch.from_numpy(c.table).cuda()
    c.d_moving = torch.from_numpy(c.moving).cuda()
    # outputs, on the host and on the device: room for every pair of every configuration
    cap = N_CONF * len(pairs)
    c.cap = cap
    c.out = np.zeros(cap, dtype=abi.RESULT_DTYPE)
    c.summ = np.zeros(N_CONF, dtype=abi.SCENE_SUMMARY_DTYPE)
    c.clear = np.zeros(N_CONF, dtype=abi.SCENE_CLEARANCE_DTYPE)
    c.pairs_out = np.zeros((cap, 2), dtype=np.uint32)
    c.conf_begin = np.zeros(N_CONF + 1, dtype=np.uint64)
    c.d_out = torch.zeros(cap * 24, dtype=torch.int32, device="cuda")
    c.d_summ = torch.zeros(N_CONF * 6, dtype=torch.int32, device="cuda")
    c.d_pairs = torch.zeros(cap * 2, dtype=torch.int32, device="cuda")
    c.d_conf_begin = torch.zeros(N_CONF + 1, dtype=torch.int64, device="cuda")
    c.d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.creq, c.dreq = abi.default_collision_request(), abi.default_distance_request()
    c.n_listed = C.c_size_t(0)
    c.n_eval = (C.c_size_t * 2)(0, 0)
    c.abi, c.d, c.pkg = abi, d, pkg
    return c


@pytest.fixture(scope="module")
def ctx(pkg, torch_cuda):
    c = make_ctx(pkg, torch_cuda)
    yield c
    for s in (c.plain, c.env, c.env32, c.stale):
        s.close()
    c.lib.close()
    c.lib2.close()


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _args(c, family):
    """the arguments of a call of the family that is not refused, by name, in the order of the C prototype"""
    p, sz, dbl = c.abi.ptr, C.c_size_t, C.c_double
    env = "env" in family
    scene = c.env if env else c.plain
    table, d_table = (c.moving, c.d_moving) if env else (c.table, c.d_table)
    if family in ("nearest", "nearest_self", "nearest_env"):
        out = c.summ if family == "nearest" else c.clear
        return [("scene", scene), ("table", p(table)), ("n_conf", sz(N_CONF)), ("req", C.byref(c.dreq)), ("upper", dbl(np.inf)), ("out", p(out)),
                ("min_records", None), ("n_evaluated", c.n_eval)]
    if family in ("self_pairs", "env_pairs"):
        return [("scene", scene), ("table", p(table)), ("n_conf", sz(N_CONF)), ("inflate", dbl(10.0)), ("pairs", p(c.pairs_out)), ("capacity", sz(c.cap)),
                ("conf_begin", p(c.conf_begin)), ("count", C.byref(c.n_listed))]
    if family in ("self_pairs_device", "env_pairs_device"):
        return [("scene", scene), ("table", _dp(d_table)), ("n_conf", sz(N_CONF)), ("inflate", dbl(10.0)), ("pairs", _dp(c.d_pairs)), ("capacity", sz(c.cap)),
                ("conf_begin", _dp(c.d_conf_begin)), ("count", _dp(c.d_count)), ("stream", C.c_void_p(0))]
    if family in ("collide_pairs_device", "collide_env_pairs_device"):  # an empty list of the right shape: the call would launch the summary init only
        return [("scene", scene), ("table", _dp(d_table)), ("n_conf", sz(N_CONF)), ("list", _dp(c.d_pairs)), ("n_listed", sz(0)),
                ("list_conf_begin", _dp(c.d_conf_begin)), ("req", C.byref(c.creq)), ("out", _dp(c.d_out)), ("summary", _dp(c.d_summ)), ("gin", None),
                ("gout", None), ("stream", C.c_void_p(0))]
    assert family in ("collide_self", "collide_env")
    return [("scene", scene), ("table", p(table)), ("n_conf", sz(N_CONF)), ("inflate", dbl(10.0)), ("req", C.byref(c.creq)), ("out", p(c.out)),
            ("capacity", sz(c.cap)), ("pairs", p(c.pairs_out)), ("conf_begin", p(c.conf_begin)), ("summary", p(c.summ)), ("gin", None), ("gout", None),
            ("count", C.byref(c.n_listed))]


# A family's refusals, the one that wins first: (label, the arguments it changes, the return code, the text -- {who}: the entry point).
# Codes: 1 HFCL_ERR_INVALID_ARGUMENT, 5 HFCL_ERR_LIMIT.
def _case(label, changes, text, code=1):
    return (label, changes, code, text)


_NULL = _case(NULL, {"scene": NULL}, "{who}: null scene")
_STALE = _case(STALE, {"scene": STALE}, "{who}: the library's shapes were replaced (hfcl_lib_set_shapes) after this scene was created; create a new scene")
_ENVS = [_case(NO_ENV, {"scene": NO_ENV}, "{who}: the scene has no environment (hfcl_scene_set_environment)"),
         _case(ENV32, {"scene": ENV32}, "{who}: the environment was set in fp32 (hfcl_scene_set_environment_f32), this call is of the other precision; "
                                        "the two pose formats are not converted into each other")]
_NAN = _case("NaN upper_bound", {"upper": C.c_double(NAN)}, "{who}: upper_bound is NaN")
_REQ = _case("null request", {"req": None}, "null request")
_TABLE = _case("null table", {"table": None}, "{who}: null pose table")
_INFLATE = _case("bad inflate", {"inflate": C.c_double(-1.0)}, "{who}: inflate must be >= 0 (and not NaN)")
_COUNT = _case("null count", {"count": None}, "{who}: null count")
_BOTH = _case("records and summaries both null", {"out": None, "summary": None}, "{who}: records and summaries both NULL")
_NO_LIST = _case("null list", {"list": None, "n_listed": C.c_size_t(3)}, "{who}: null list / conf_begin")


def _out(words):
    return _case("null output", {"out": None}, "{who}: " + words)


def _no_conf(what):
    return _case("list entries without a configuration", {"n_conf": C.c_size_t(0), "n_listed": C.c_size_t(3)},
                 "{who}: list entries without a configuration or " + what)


def _capacity(text):  # (inflate 10 lists every pair: 2 x 15, and 2 x (6 + 8) with four moving objects)
    return _case("capacity below the count", {"capacity": C.c_size_t(1)}, "{who}: " + text, code=5)


FAMILIES = {
    "nearest": ("hfcl_scene_nearest", [_NAN, _NULL, _REQ, _out("null summaries"), _STALE, _TABLE]),
    "nearest_self": ("hfcl_scene_nearest_self", [_NAN, _NULL, _REQ, _out("null output"), _STALE, _TABLE]),
    "nearest_env": ("hfcl_scene_nearest_env", [_NAN, _NULL, _REQ, _out("null output"), _STALE] + _ENVS + [_TABLE]),
    "self_pairs": ("hfcl_scene_self_pairs", [_NULL, _STALE, _TABLE, _INFLATE, _COUNT, _capacity("30 pairs are listed, the list holds 1")]),
    "self_pairs_device": ("hfcl_scene_self_pairs_device", [_NULL, _STALE, _TABLE, _INFLATE, _COUNT]),
    "env_pairs": ("hfcl_scene_env_pairs", [_NULL, _STALE] + _ENVS + [_TABLE, _INFLATE, _COUNT, _capacity("28 pairs are listed, the list holds 1")]),
    "env_pairs_device": ("hfcl_scene_env_pairs_device", [_NULL, _STALE] + _ENVS + [_TABLE, _INFLATE, _COUNT]),
    "collide_pairs_device": ("hfcl_scene_collide_pairs_device", [_NULL, _REQ, _BOTH, _STALE, _no_conf("an object"), _TABLE, _NO_LIST]),
    "collide_env_pairs_device": ("hfcl_scene_collide_env_pairs_device",
                                 [_NULL, _REQ, _BOTH, _STALE] + _ENVS + [_no_conf("a moving object"), _TABLE, _NO_LIST]),
    "collide_self": ("hfcl_scene_collide_self",
                     [_NULL, _REQ, _BOTH, _STALE, _TABLE, _INFLATE, _COUNT, _capacity("30 queries survive, the outputs hold 1")]),
    "collide_env": ("hfcl_scene_collide_env",
                    [_NULL, _REQ, _BOTH, _STALE] + _ENVS + [_TABLE, _INFLATE, _COUNT, _capacity("28 queries survive, the outputs hold 1")]),
}


def _cases(family):
    return {label: changes for label, changes, _, _ in FAMILIES[family][1]}


def expected(family, label):
    who = FAMILIES[family][0]
    return next((code, text.format(who=who)) for l, _, code, text in FAMILIES[family][1] if l == label)


def observe(c, family, labels):
    """(return code, error text) of the family's call with the changes of every label in `labels`"""
    fn_name = FAMILIES[family][0]
    changes = {}
    for label in labels:
        changes.update(_cases(family)[label])
    scenes = {NULL: None, STALE: c.stale, NO_ENV: c.plain, ENV32: c.env32}
    args = []
    for name, value in _args(c, family):
        value = changes.get(name, value)
        if name == "scene":
            value = scenes[value] if isinstance(value, str) else value
            value = value._h if value is not None else None
        args.append(value)
    rc = getattr(c.d, fn_name)(*args)
    return int(rc), c.pkg.engine.last_error()


def combinable(family, a, b):
    """two refusals of a family that one call can have at once: they change different arguments"""
    cases = _cases(family)
    return not set(cases[a]) & set(cases[b])


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_refusal_code_and_text(ctx, family):
    assert observe(ctx, family, [])[0] == ctx.abi.OK, ctx.pkg.engine.last_error()  # the family's own call is not refused
    for label in _cases(family):
        got = observe(ctx, family, [label])
        print(family, label, got)
        assert got == expected(family, label), (family, label)
        assert got[0] != ctx.abi.OK


@pytest.mark.parametrize("family", list(FAMILIES))
def test_of_two_refusals_the_earlier_wins(ctx, family):
    labels = list(_cases(family))
    n = 0
    for a, b in itertools.combinations(labels, 2):  # (a stands before b)
        if combinable(family, a, b):
            assert observe(ctx, family, [a, b]) == expected(family, a), (family, a, b)
            n += 1
    assert n >= len(labels)
