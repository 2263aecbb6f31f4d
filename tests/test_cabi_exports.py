"""The C-ABI boundary on a machine without a GPU: the real libcyclevae_hip.so (hipcc, gfx950) loads, exports every function
include/cyclevae_hip.h declares, the ctypes binding lists exactly those, and an ABI/size query answers (no compute calls)."""
import ctypes
import os
import re

import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cyclevae-vc_amd", "libcyclevae_hip.so")


def declared_functions():
    text = open(os.path.join(ROOT, "include", "cyclevae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cvae_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_library_agree():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    names = declared_functions()
    assert len(names) >= 20
    assert sorted(_cabi.EXPORTS) == names, (sorted(set(names) - set(_cabi.EXPORTS)), sorted(set(_cabi.EXPORTS) - set(names)))
    assert set(_cabi.ADDITIVE) <= set(_cabi.EXPORTS)      # optional when an older build of the same ABI loads, never in this one
    lib = ctypes.CDLL(LIB)
    for n in names:
        assert hasattr(lib, n), "libcyclevae_hip.so does not export " + n
    lib.cvae_abi_version.restype = ctypes.c_int
    assert lib.cvae_abi_version() == _cabi.ABI_VERSION


def test_size_queries_answer_without_a_gpu():
    import pytest
    lib = _cabi.CvaeLib(LIB)
    d = lib.desc(54, 64, 1024, 3, 2, True, False)
    assert lib.prepared_bytes(d) > 4 * 5_000_000                # at least the folded weights of a 5.2 M-parameter net
    assert lib.pass_workspace_bytes(d, 64, 80) > 64 * 80 * 1024 * 4
    bad = lib.desc(54, 64, 1000, 3, 2, True, False)             # H not a multiple of 16: refused, with a message
    with pytest.raises(_cabi.CvaeError):
        lib.prepared_bytes(bad)
    assert lib.lib.cvae_last_error_string() not in (None, b"")


def test_deep_plan_query_answers_without_a_gpu():
    """cvae_plan_pass_deep_tiles on the shipped library: the path cvae_plan_pass_deep reports, Bp, and a tiling that covers Bp (which
    one depends on the device's CU count: tests/stacked_cases.py holds every case to the MI355X's)."""
    import pytest
    lib = _cabi.CvaeLib(LIB)
    d = lib.desc(6, 8, 64, 3, 2, True, False)
    for flags in (0, _cabi.FLAG_PERSISTENT, _cabi.FLAG_PERSISTENT | _cabi.FLAG_GENERIC_STEP):
        path, Bp, rts, tiles = lib.plan_pass_deep_tiles(d, 2, 70, 3, flags)
        assert path == lib.plan_pass_deep(d, 2, 70, 3, flags) and Bp == 96
        if path == _cabi.DEEP_RESIDENT:
            assert 1 <= rts <= 3 and tiles == -(-3 // rts) <= 4
        else:
            assert (rts, tiles) == (1, 6)
    with pytest.raises(_cabi.CvaeError):
        lib.plan_pass_deep_tiles(d, 1, 70, 3, 0)


def test_train_plan_query_answers_without_a_gpu():
    """cvae_plan_train_pass on the shipped library: Bp, forms of the enum's range, a tiling that covers Bp in both directions (which
    one depends on the device's CU count: tests/train_cases.py holds every case to the MI355X's), per-step launches for one frame."""
    import pytest
    lib = _cabi.CvaeLib(LIB)
    assert "cvae_plan_train_pass" in _cabi.ADDITIVE and len(_cabi.TRAIN_PLAN_FIELDS) == 12
    d = lib.desc(6, 8, 64, 3, 2, True, False)
    p = lib.plan_train_pass(d, 70, 3)
    assert list(p) == list(_cabi.TRAIN_PLAN_FIELDS) and p["Bp"] == 96
    assert _cabi.TRAIN_FWD_LL < p["fwd"] <= _cabi.TRAIN_FWD_STEPS and _cabi.TRAIN_BWD_LL < p["bwd"] <= _cabi.TRAIN_BWD_STEPS
    if p["fwd"] != _cabi.TRAIN_FWD_STEPS:
        assert p["fwd_rts"] >= 1 and p["fwd_rts"] * p["fwd_tiles"] >= (3 if p["fwd"] == _cabi.TRAIN_FWD_X3 else 6) and p["fwd_full_writes"] == 1
    if p["bwd"] != _cabi.TRAIN_BWD_STEPS:
        assert p["bwd_rts"] >= 1 and p["bwd_rts"] * p["bwd_tiles"] >= min(6, p["bwd_per_launch"] or 6) and p["bwd_tiles"] <= 2
    one = lib.plan_train_pass(d, 70, 1)
    assert (one["fwd"], one["bwd"], one["fwd_tiles"], one["bwd_tiles"]) == (_cabi.TRAIN_FWD_STEPS, _cabi.TRAIN_BWD_STEPS, 0, 0)
    assert lib.plan_train_pass(lib.desc(6, 8, 48, 3, 2, True, False), 5, 4)["fwd"] == _cabi.TRAIN_FWD_STEPS      # no persistent form off 64 / 1024
    with pytest.raises(_cabi.CvaeError):
        lib.plan_train_pass(d, 0, 3)


def test_recurrent_kernels_do_not_spill():
    """hipcc's kernel-resource-usage remarks of the shipped build: the all-resident recurrent kernels of the default paths use no
    scratch (a private segment puts a ~240 us gap in front of every launch on MI355X and turns register traffic into memory
    traffic), and run at one wave per SIMD with the 512 registers that assumes."""
    import __graft_entry__
    if not os.path.exists(__graft_entry__.RESOURCES) or os.path.getmtime(__graft_entry__.RESOURCES) < os.path.getmtime(LIB):
        __graft_entry__.build(force=True)
    text = open(__graft_entry__.RESOURCES).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", text)[1:]
    assert len(blocks) > 100, "no resource remarks in " + __graft_entry__.RESOURCES
    seen = set()
    for b in blocks:
        name = b.split()[0]
        hot = [k for k in ("k_gru_steps_v6", "k_gru_steps_v5", "k_gru_steps_ll", "k_train_fwd_steps_x3", "k_train_fwd_steps_w3", "k_train_fwd_steps_h", "k_train_fwd_steps_ll",
                           "k_train_bwd_steps", "k_outproj_v6", "k_prologue") if k in name]
        if not hot:
            continue
        seen.add(hot[0])
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, "%s spills %d bytes per lane" % (name, scratch)
    assert {"k_gru_steps_v6", "k_gru_steps_ll", "k_train_fwd_steps_x3", "k_train_fwd_steps_w3", "k_train_bwd_steps"} <= seen
    assert any("k_train_bwd_steps_w3" in b.split()[0] for b in blocks)          # (covered by the k_train_bwd_steps prefix above)


def test_option_table_matches_the_library():
    """The option table in include/cyclevae_hip.h lists exactly the names and defaults of g_opt (cvae_lib.hip), and a fresh context
    reports those defaults."""
    from emu_util import emu_lib
    text = open(os.path.join(ROOT, "include", "cyclevae_hip.h")).read()
    table = text[text.index(" *   name                default  meaning"):text.index("int cvae_set_option(")]
    documented = {n: int(v) for n, v in re.findall(r'^ \*   "([a-z0-9_]+)"\s+(-?\d+)\s', table, re.M)}
    src = open(os.path.join(ROOT, "cyclevae-vc_amd", "csrc", "cvae_lib.hip")).read()
    g_opt = src[src.index("const OptEntry g_opt[OPT_COUNT] = {"):]
    g_opt = g_opt[:g_opt.index("\n};")]
    defined = {n: int(v) for n, v in re.findall(r'^\s*\{"([a-z0-9_]+)",\s*(-?\d+)\}', g_opt, re.M)}
    assert len(defined) >= 30
    assert documented == defined, ({k: documented.get(k) for k in set(documented) ^ set(defined)},
                                   {k: (documented[k], defined[k]) for k in set(documented) & set(defined) if documented[k] != defined[k]})
    lib = emu_lib()
    lib.reset_options()
    for name, dflt in defined.items():
        assert lib.get_option(name) == dflt, name
