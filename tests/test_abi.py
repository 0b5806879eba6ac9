"""C-ABI boundary checks that run without a GPU.

The first part reads include/crowdnav.h (comments stripped) and holds the Python copies against it without loading
anything: _lib.SIGNATURES against every prototype (parameter count, pointer / integer / floating kind, size and
signedness of every parameter and of the return type), the nine struct mirrors of abi.py against the header's
structs (field names in order, each field's kind, size and array length, the offsets natural alignment gives), and
abi's constants against the #defines. The second part loads the native library: it exports every declared symbol
and agrees with the Python layout mirror (no compute calls)."""
import ctypes
import os
import re

import pytest

from crowdnav_dsrnn_amd import abi, _lib
from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "crowdnav.h")
PROTOTYPE = re.compile(r"^((?:const\s+)?[\w ]+?\**)\s*\b(cn_\w+)\s*\(([^;{}]*?)\)\s*;", re.M)
# C scalar -> (kind, sizeof, signed)
C_SCALARS = {"int": ("int", 4, True), "int32_t": ("int", 4, True), "uint32_t": ("int", 4, False),
             "int64_t": ("int", 8, True), "long long": ("int", 8, True), "float": ("float", 4, True),
             "double": ("float", 8, True)}
INT64_RETURNS = {"cn_gru_bias_blocks", "cn_wgrad_work_elems", "cn_gru_bwd_seq_work_elems", "cn_gru_bias_work_elems"}
POINTER_RETURNS = {"cn_last_error": ctypes.c_char_p, "cn_version": ctypes.c_char_p,
                   "cn_state_device_ptr": ctypes.c_void_p}
STRUCTS = {"cn_config": abi.CnConfig, "cn_gru_step_seg": abi.GruStepSeg, "cn_gru_seq_fwd": abi.GruSeqFwd,
           "cn_gru_seq_bwd": abi.GruSeqBwd, "cn_dwa_params": abi.DwaParams, "cn_mix_ctl": abi.CnMixCtl,
           "cn_rollout_out": abi.RolloutOut, "cn_rollout_noise": abi.RolloutNoise,
           "cn_rollout_lidar": abi.RolloutLidar}


def declared_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(cn_[a-z_0-9]+)\s*\(", txt)) - {"cn_engine"})


def header_text():
    """include/crowdnav.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def prototypes(txt):
    """{name: (return type, [parameter declarations])} of every prototype, in the header's order."""
    out = {}
    for ret, name, params in PROTOTYPE.findall(txt):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def _ctype_kind(t):
    """(kind, sizeof, signed) of a ctypes scalar; ("pointer", 8, None) of c_void_p / c_char_p / a POINTER(..);
    None of anything else (None itself, a structure by value, an array)."""
    if isinstance(t, type) and issubclass(t, ctypes._Pointer) or t in (ctypes.c_void_p, ctypes.c_char_p):
        return ("pointer", ctypes.sizeof(t), None)
    code = getattr(t, "_type_", None) if isinstance(t, type) and issubclass(t, ctypes._SimpleCData) else None
    if isinstance(code, str) and code in "bBhHiIlLqQ":
        return ("int", ctypes.sizeof(t), code.islower())
    if isinstance(code, str) and code in "fd":
        return ("float", ctypes.sizeof(t), True)
    return None


def _type_mismatch(ctext, bound):
    """Why `bound` (a ctypes type or None) does not bind the C type `ctext` ("int64_t", "const float *", "void"),
    or None if it does."""
    if "*" in ctext:
        want = ("pointer", ctypes.sizeof(ctypes.c_void_p), None)
    elif ctext == "void":
        return None if bound is None else "void bound to %r" % (bound,)
    else:
        want = C_SCALARS.get(ctext.replace("const ", ""))
        if want is None:
            return "C type %r is not one this check knows" % ctext
    got = _ctype_kind(bound)
    return None if got == want else "%s is %r in C, bound to %r %r" % (ctext, want, bound, got)


def signature_mismatches(txt, table):
    """Every disagreement between the prototypes of the header text `txt` and `table` (name -> (restype,
    argtypes), as _lib.SIGNATURES), as a list of "name: what" strings."""
    protos = prototypes(txt)
    bad = ["%s: in the header, not in the table" % n for n in protos if n not in table]
    bad += ["%s: in the table, not in the header" % n for n in table if n not in protos]
    for name, (ret, params) in protos.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        why = _type_mismatch(ret, restype)
        if why:
            bad.append("%s: return: %s" % (name, why))
        if len(params) != len(argtypes):
            bad.append("%s: %d parameters in C, %d argtypes" % (name, len(params), len(argtypes)))
            continue
        for k, (p, a) in enumerate(zip(params, argtypes)):
            ctext = p if "*" in p else p.rsplit(" ", 1)[0]   # (a scalar: drop the parameter's name)
            why = _type_mismatch(ctext, a)
            if why:
                bad.append("%s: parameter %d (%s): %s" % (name, k, p, why))
    return bad


def header_structs(txt):
    """{struct name: [(field, C type, is pointer, array length or None)]} of every struct the header defines."""
    defines = dict(re.findall(r"^#define (CN_\w+) (\d+)\s*$", txt, re.M))
    out = {}
    for name, body in re.findall(r"\bstruct\s+(cn_\w+)\s*\{(.*?)\}", txt, re.S):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *rest = [d.strip() for d in decl.split(",")]
            m = re.fullmatch(r"(?:const )?([\w ]+?) ?(\**) ?(\w+)(?:\[(\w+)\])?", first)
            assert m, (name, decl)
            ctype = m.group(1)
            declarators = [m.groups()[1:]] + [re.fullmatch(r"(\**) ?(\w+)(?:\[(\w+)\])?", d).groups() for d in rest]
            for stars, field, n in declarators:
                fields.append((field, ctype, bool(stars), None if n is None else int(defines.get(n, n))))
        out[name] = fields
    return out


@pytest.fixture(scope="module")
def L():
    from crowdnav_dsrnn_amd import build

    build.build()
    return _lib.lib()


def test_header_declares_expected_api():
    """Every cn_x( of the header, its comments included, is a prototype the parser reads (one it cannot read fails
    here instead of shrinking the checks below), and the table has exactly those names, in the header's order."""
    assert set(declared_symbols()) == set(_lib.EXPORTED)
    parsed = list(prototypes(header_text()))
    assert len(parsed) == len(set(parsed))
    assert set(parsed) == set(declared_symbols())
    assert parsed == list(_lib.SIGNATURES) == _lib.EXPORTED


def test_signatures_match_header_prototypes():
    """Every parameter and return type of _lib.SIGNATURES binds its prototype: a pointer to c_void_p, c_char_p or a
    POINTER(..), a scalar to a ctypes scalar of the same kind, size and signedness, void to None, counts equal."""
    assert signature_mismatches(header_text(), _lib.SIGNATURES) == []


def test_wide_return_types_are_bound():
    """The functions whose result a forgotten restype would cut to 32 bits: the header still has each (so the check
    above cannot have gone vacuous for them) and the table binds int64_t to c_int64 and the pointers as such."""
    protos = prototypes(header_text())
    assert {n for n, (ret, _) in protos.items() if ret == "int64_t"} == INT64_RETURNS
    assert {n for n, (ret, _) in protos.items() if "*" in ret} == set(POINTER_RETURNS)
    assert {protos[n][0] for n in POINTER_RETURNS} == {"const char *", "const void *"}
    assert {n for n, (ret, _) in protos.items() if ret == "void"} == {"cn_destroy"}
    for n in INT64_RETURNS:
        assert _lib.SIGNATURES[n][0] is ctypes.c_int64, n
    for n, t in POINTER_RETURNS.items():
        assert _lib.SIGNATURES[n][0] is t, n
    assert _lib.SIGNATURES["cn_destroy"][0] is None


def test_signature_check_reports_a_narrowed_argument_and_a_dropped_restype():
    """The checker can fail: an int64_t bound as c_int, and an int64_t / pointer result left at ctypes' default
    restype (c_int), are each reported, and nothing else is."""
    txt = header_text()
    table = dict(_lib.SIGNATURES)
    restype, argtypes = table["cn_step_seq"]
    k = argtypes.index(ctypes.c_int64)
    table["cn_step_seq"] = (restype, argtypes[:k] + [ctypes.c_int] + argtypes[k + 1:])
    bad = signature_mismatches(txt, table)
    assert len(bad) == 1 and bad[0].startswith("cn_step_seq: parameter %d (int64_t action_stride)" % k), bad

    for name in ("cn_gru_bias_blocks", "cn_state_device_ptr"):
        table = dict(_lib.SIGNATURES)
        table[name] = (ctypes.c_int, table[name][1])
        bad = signature_mismatches(txt, table)
        assert len(bad) == 1 and bad[0].startswith("%s: return:" % name), bad

    table = dict(_lib.SIGNATURES)
    table["cn_wgrad"] = (table["cn_wgrad"][0], table["cn_wgrad"][1][:-1])
    del table["cn_gae"]
    bad = signature_mismatches(txt, table)   # a parameter short, and a prototype without an entry
    assert sorted(b.split(":")[0] for b in bad) == ["cn_gae", "cn_wgrad"], bad


def test_library_exports_every_declared_symbol(L):
    for sym in declared_symbols():
        assert hasattr(L, sym), sym


def test_struct_set_matches_header():
    assert set(header_structs(header_text())) == set(STRUCTS)
    for name in ("GruSeqFwd", "GruSeqBwd", "GruStepSeg", "RolloutOut", "RolloutNoise", "RolloutLidar", "DwaParams",
                 "ROLLOUT_OBS_EVERY_STEP"):
        assert getattr(_lib, name) is getattr(abi, name), name   # (_lib keeps the names its callers use)


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_structs_match_header(cname):
    """A struct mirror lists the header's fields in its order, each of the header type's kind, size, signedness and
    array length, at the offset natural alignment gives it: ctypes then lays it out as the compiler does."""
    py, fields = STRUCTS[cname], header_structs(header_text())[cname]
    assert [f for f, _, _, _ in fields] == [f[0] for f in py._fields_]
    assert not hasattr(py, "_pack_")
    off = align = 0
    for (field, ctext, is_ptr, n), (_, bound) in zip(fields, py._fields_):
        if n is not None:
            assert issubclass(bound, ctypes.Array) and bound._length_ == n, field
            bound = bound._type_
        assert _type_mismatch(ctext + " *" if is_ptr else ctext, bound) is None, field
        size = 8 if is_ptr else C_SCALARS[ctext][1]
        off = (off + size - 1) // size * size
        assert getattr(py, field).offset == off and getattr(py, field).size == size * (n or 1), field
        off, align = off + size * (n or 1), max(align, size)
    assert ctypes.sizeof(py) == (off + align - 1) // align * align
    if cname in ("cn_gru_seq_fwd", "cn_gru_seq_bwd", "cn_gru_step_seg"):
        assert ctypes.sizeof(py) == 8 * len(fields)   # (every field int64_t or a pointer)


def test_constants_match_header():
    """Every #define CN_<X> <integer> that abi mirrors as <X> has the header's value; the families the host side
    uses are all mirrored; abi.SCENARIOS[k] is the CN_SC_* name of value k."""
    defines = {k: int(v) for k, v in re.findall(r"^#define CN_(\w+) \(?(-?\d+)\)?\s*$", header_text(), re.M)}
    assert len(defines) == len(re.findall(r"^#define CN_", header_text(), re.M))   # (every one is an integer)
    for name, value in defines.items():
        if hasattr(abi, name):
            assert getattr(abi, name) == value, name
    families = ("EV_", "INFO_", "PHASE_", "RNG_", "ROBOT_", "POLICY_", "SCMODE_")
    required = [n for n in defines if n.startswith(families)]
    required += ["HOLONOMIC", "UNICYCLE", "MAX_SCENARIOS", "ROLLOUT_OBS_EVERY_STEP"]
    for fam in families:
        assert any(n.startswith(fam) for n in required), fam
    assert "INFO_K" in required
    for name in required:
        assert name in defines and hasattr(abi, name), name
    scenarios = {v: k[3:].lower() for k, v in defines.items() if k.startswith("SC_")}
    assert abi.SCENARIOS == [scenarios[k] for k in range(len(scenarios))]
    assert len(abi.SCENARIOS) <= abi.MAX_SCENARIOS


def test_gru_seq_rejects_bad_arguments_without_launching(L):
    segs = (_lib.GruSeqFwd * 3)()
    assert L.cn_gru_fwd_seq(None, 4, 256, 3, segs) != 0      # at most two GRUs per call
    assert L.cn_gru_fwd_seq(None, 4, 96 + 4, 1, segs) != 0   # H % 32
    assert L.cn_gru_fwd_seq(None, 4, 256, 1, segs) != 0      # B = 0, null operands
    bsegs = (_lib.GruSeqBwd * 2)()
    bsegs[0].B, bsegs[1].B = 20480, 2048
    # workspace: bias partials of 128-row tiles ((160 + 16) x 4H per step) + the reduction's 64 x 4H
    assert L.cn_gru_bwd_seq_work_elems(3, 256, 2, bsegs) == (3 * 176 + 64) * 1024
    bsegs[0].B = 2048   # 16 x 4 tiles of 128 rows < 256 CUs: split-K on 32-row tiles (64 per step)
    assert L.cn_gru_bwd_seq_work_elems(2, 128, 1, bsegs) == (2 * 64 + 64) * 512
    assert L.cn_gru_bwd_seq(None, 0, 256, 1, bsegs, None, 0) != 0     # T = 0
    assert L.cn_gru_bwd_seq(None, 4, 256, 1, bsegs, None, 0) != 0
    assert b"cn_gru_bwd_seq" in L.cn_last_error()
    # a workspace below the size for the current device is rejected before any launch (the split-K
    # choice follows the device's CU count; dummy 16-byte aligned operands are never dereferenced)
    one = (_lib.GruSeqBwd * 1)()
    one[0] = _lib.GruSeqBwd(2048, 16, 32, 48, 64, 80, 96, 112, 128, 144)
    need = L.cn_gru_bwd_seq_work_elems(2, 128, 1, one)
    assert L.cn_gru_bwd_seq(None, 2, 128, 1, one, 4096, need - 1) != 0
    assert b"workspace smaller" in L.cn_last_error()
    # masked-state ring: nh >= 2 when T > 1 (a step reads hm[t % nh] while other workgroups write
    # hm[(t + 1) % nh]); nh == T with save (the backward reads every step's hm). Rejected before any launch
    # (non-null dummy addresses, 16-byte aligned, are never dereferenced)
    seg = (_lib.GruSeqFwd * 1)()
    seg[0] = _lib.GruSeqFwd(64, 16, 32, 48, 64, 80, 96, None, 1, None, None, None, 0)
    assert L.cn_gru_fwd_seq(None, 4, 256, 1, seg) != 0 and b"nh >= 2" in L.cn_last_error()
    seg[0].nh, seg[0].save = 2, 112
    assert L.cn_gru_fwd_seq(None, 4, 256, 1, seg) != 0 and b"nh == T" in L.cn_last_error()


def test_gru_step_entry_points_reject_bad_arguments_without_launching(L):
    """cn_gru_fwd_fused, cn_gru_fwd_step_group, cn_gru_bwd_step_bias / _gates and cn_gru_bias_reduce turn down
    sizes, layouts and alignments their kernels do not serve before any launch (non-null dummy addresses, 16-byte
    aligned unless the case says otherwise, are never dereferenced), each naming itself in cn_last_error()."""
    def rejected(rc, who):
        return rc != 0 and who in L.cn_last_error()

    # cn_gru_fwd_fused(stream, B, H, gi, hm, w_hh, b_hh, m_next, h_out, hm_next, save, h_out2, g2, ld2)
    fused = b"cn_gru_fwd_fused"
    assert rejected(L.cn_gru_fwd_fused(None, 64, 48, 16, 32, 48, 64, None, 80, None, None, None, 1, 0), fused)    # H % 32
    assert rejected(L.cn_gru_fwd_fused(None, 64, 64, 16, 36, 48, 64, None, 80, None, None, None, 1, 0), fused)    # hm + 4
    assert b"16-byte aligned" in L.cn_last_error()
    assert rejected(L.cn_gru_fwd_fused(None, 64, 64, 16, 32, 48, 64, None, 80, None, None, 96, 0, 640), fused)    # g2 = 0
    assert rejected(L.cn_gru_fwd_fused(None, 64, 64, 16, 32, 48, 64, None, 80, None, None, 96, 5, 319), fused)    # ld2 < g2 H
    assert b"ld2 >= g2 * H" in L.cn_last_error()

    # cn_gru_step_seg: B, gi, x, w_ih, b_ih, F, hm, w_hh, b_hh, h_out, h_out2, g2, ld2
    group = b"cn_gru_fwd_step_group"
    with_gi = _lib.GruStepSeg(64, 16, None, None, None, 0, 32, 48, 64, 80, None, 1, 0)
    with_x = _lib.GruStepSeg(64, None, 16, 96, 112, 64, 32, 48, 64, 80, None, 1, 0)
    segs = (_lib.GruStepSeg * 3)(with_gi, with_x, with_gi)
    assert rejected(L.cn_gru_fwd_step_group(None, 256, 2, segs), group)                    # one GRU gi, the other x
    assert b"every GRU" in L.cn_last_error()
    assert rejected(L.cn_gru_fwd_step_group(None, 256, 3, segs), group)                    # nseg = 3
    one = (_lib.GruStepSeg * 1)(with_x)
    one[0].F = 48
    assert rejected(L.cn_gru_fwd_step_group(None, 256, 1, one), group)                     # x with F % 32 != 0
    assert b"F % 32" in L.cn_last_error()
    one[0] = with_gi
    one[0].w_hh = 52
    assert rejected(L.cn_gru_fwd_step_group(None, 256, 1, one), group)                     # a misaligned array
    assert b"16-byte aligned" in L.cn_last_error()

    # the bias-folding step kernels serve H in {64, 128, 256} only; the reduction needs rows
    assert rejected(L.cn_gru_bwd_step_bias(None, 16, 96, 16, None, None, 32, 48, 64, 80, 96), b"cn_gru_bwd_step_bias")
    assert rejected(L.cn_gru_bwd_step_gates(None, 16, 96, 16, None, None, 32, 48, 64, 80), b"cn_gru_bwd_step_gates")
    assert rejected(L.cn_gru_bias_reduce(None, 0, 64, 16, 32, 48, 64), b"cn_gru_bias_reduce")


def test_step_seq_and_graph_census_reject_bad_arguments(L):
    """cn_step_seq / cn_graph_node_counts validate their arguments before touching the GPU."""
    assert L.cn_step_seq(None, None, 4, None, 0, *([None] * 9)) != 0
    counts = (ctypes.c_int64 * 4)()
    assert L.cn_graph_node_counts(None, counts, 4, None) != 0
    assert L.cn_graph_node_counts(ctypes.c_void_p(16), counts, 33, None) != 0   # n > 32


def test_config_struct_size_matches(L):
    # a validate call on a deliberately invalid config only reads the struct (no GPU work)
    c = abi.CnConfig()
    assert L.cn_config_validate(ctypes.byref(c)) != 0
    assert b"num_envs" in L.cn_last_error()


def test_state_layout_matches_python_mirror(L):
    cfg = make_cn_config(clone_config(Config()), num_envs=37)
    for N, vis in ((5, 0), (10, 0), (12, 0), (25, 1), (1, 0)):
        cfg.human_num, cfg.robot_visible = N, vis
        offs = (ctypes.c_int64 * 64)()
        tot = ctypes.c_int64()
        assert L.cn_state_layout_offsets(ctypes.byref(cfg), offs, ctypes.byref(tot)) == 0
        lay, total = abi.state_layout(37, N, vis)
        assert total == tot.value
        for k, (name, _, _) in enumerate(abi.STATE_FIELDS):
            assert lay[name][0] == offs[k], name
            nm, tc, ck = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
            assert L.cn_state_field_info(k, ctypes.byref(nm), ctypes.byref(tc), ctypes.byref(ck)) == 0
            assert nm.value.decode() == name


def test_validate_rejects_unsupported(L):
    cfg = make_cn_config(clone_config(Config()), num_envs=8)
    assert L.cn_config_validate(ctypes.byref(cfg)) == 0
    bad = cfg.copy()
    bad.human_num = 40
    assert L.cn_config_validate(ctypes.byref(bad)) != 0
    bad = cfg.copy()
    bad.potential_based = 0
    assert L.cn_config_validate(ctypes.byref(bad)) != 0


def test_make_cn_config_rejects_unsupported_reference_options():
    c = clone_config(Config())
    c.sim.group_human = True
    with pytest.raises(UnsupportedConfig):
        make_cn_config(c, 4)
    c = clone_config(Config())
    c.robot.policy = "cadrl"
    with pytest.raises(UnsupportedConfig):
        make_cn_config(c, 4)
    c = clone_config(Config())        # the LiDAR / ConvGRU observation is served (cn_lidar_obs)
    c.lidar.enable = True
    c.robot.policy = "convgru"
    make_cn_config(c, 4)


def test_make_cn_config_defaults_follow_make_env():
    c = make_cn_config(clone_config(Config()), num_envs=12)
    assert c.phase == abi.PHASE_TRAIN and c.nenv == 12   # envs.py:69-73
    c1 = make_cn_config(clone_config(Config()), num_envs=1)
    assert c1.phase == abi.PHASE_TEST
    assert abs(c.robot_fov - 2 * 3.141592653589793) < 1e-12


def test_build_deps_cover_every_included_file():
    """build.DEPS (what CN_SRC_HASH is taken over) holds every file the compiled sources reach through
    `#include "..."`, followed recursively: a header left out would let a stale library pass for a fresh one.
    The list is SOURCES first, then the headers sorted, without duplicates (a deterministic hash)."""
    from crowdnav_dsrnn_amd import build

    reached, todo = set(), list(build.SOURCES)
    while todo:
        f = os.path.realpath(todo.pop())
        if f in reached:
            continue
        reached.add(f)
        assert os.path.exists(f), f
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M):
            todo.append(os.path.join(os.path.dirname(f), inc))
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert any(os.sep + "engine" + os.sep in f for f in reached)   # (the walk went into csrc/engine/)
    assert any(os.sep + "csrc" + os.sep + "policy" + os.sep in f for f in reached)   # (and into csrc/policy/)
    assert reached <= set(deps), sorted(reached - set(deps))
    assert len(set(deps)) == len(deps)
    n = len(build.SOURCES)
    assert build.DEPS[:n] == build.SOURCES
    assert build.DEPS[n:] == sorted(build.DEPS[n:])


def test_library_built_from_sources_on_disk(L):
    """The loaded library embeds the sha256 of the sources it was built from (build.py) and it equals
    the hash of the committed sources: GPU evidence produced with it belongs to this tree."""
    from crowdnav_dsrnn_amd import build

    ver = L.cn_version().decode()
    assert "CN_SRC_HASH=" + build.source_hash() in ver
    assert build.built_hash() == build.source_hash()
    assert not build.needs_build()
