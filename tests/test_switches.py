"""The environment switches of csrc/ live in one header, nlls_switches.hpp: tests/abi/switches_check.cpp includes it alone (plain g++, no HIP) and prints
what the two loaders make of this process's environment -- the defaults against the table of DESIGN.md 9, every parse rule at its boundary values, and read_upload_env
leaving the create-time fields alone.  Then three source checks: nothing else in csrc/ reads the environment, the header and the table name the same switches, and the
launch layer (nlls_launch.hpp) is the only place that sets a kernel attribute or defines the HIP error check."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
HDR = os.path.join(CSRC, "nlls_switches.hpp")
SRC = os.path.join(ROOT, "tests", "abi", "switches_check.cpp")
EXE = os.path.join(ROOT, "tests", "abi", "switches_check.out")


def _build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-o", EXE, SRC])
    return EXE


def run(env=None, *args):
    out = subprocess.run([_build(), *args], capture_output=True, text=True, env=dict(env or {}))
    assert out.returncode == 0, out.stderr
    return dict(line.split("=") for line in out.stdout.split())


def design_table():
    """rows of DESIGN.md 9: switch -> (field, default, read at)"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 9. Run-time switches"):]
    rows = re.findall(r"^\| `(NLLS_[A-Z0-9_]+)` \| `(\w+)` \| (\S+) \| (create|upload) \|", sec, flags=re.M)
    return {name: (field, default, when) for name, field, default, when in rows}


def test_defaults_are_those_of_the_design_table():
    got, table = run(), design_table()
    assert len(table) == 27 and sorted(got) == sorted(f for f, _, _ in table.values())
    for name, (field, default, _) in table.items():
        assert got[field] == default, (name, field, got[field], default)


# switch -> (field, [(text, value the field takes)]): the rules of nlls_switches.hpp at their boundaries.  "x" is text atoi reads as 0; D the default
RULES = {
    "NLLS_NO_LOOKAHEAD_SWEEP":  ("spec_on", [("1", "false"), ("1x", "false"), ("0", "true"), ("", "true"), ("x", "true"), ("-1", "true")]),
    "NLLS_MATERIALIZE":         ("mf_on", [("1", "false"), ("0", "true"), ("", "true"), ("x", "true"), ("-1", "true")]),
    "NLLS_TINY_DENSE":          ("tiny_dense_on", [("0", "false"), ("0x", "false"), ("1", "true"), ("", "true"), ("x", "true"), ("-1", "true")]),      # only a leading '0' turns it off
    "NLLS_POST_SPLIT":          ("post_fuse", [("1", "false"), ("0", "true"), ("", "true"), ("x", "true")]),
    "NLLS_ELIM_SPLIT":          ("elim_split", [("1", "true"), ("0", "false"), ("", "false"), ("x", "false")]),
    "NLLS_DENSE_STEP_BACKWARD": ("dense_fused_bwd", [("1", "false"), ("0", "true"), ("", "true"), ("x", "true")]),
    "NLLS_DENSE_T128_MIN":      ("dense_t128_min", [("1", "1"), ("0", "0"), ("-1", "-1"), ("x", "0"), ("128", "128")]),
    "NLLS_SINGLES_WAVE_MIN":    ("singles_wave_min", [("1", "1"), ("0", "D"), ("-1", "D"), ("x", "D"), ("127", "127"), ("99999999999", "99999999999")]),   # <= 0 is ignored; 64 bits
    "NLLS_NO_ARENA":            ("no_arena", [("1", "true"), ("0", "true"), ("", "true"), ("x", "true")]),                                            # set at all
    "NLLS_SWEEP_FOLD":          ("sweep_fold", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),                                                   # unset: -1 (the default)
    "NLLS_HEAVY_MAX_ENTRIES":   ("heavy_max_entries", [("127", "D"), ("128", "128"), ("0", "D"), ("1", "D"), ("-1", "D"), ("x", "D"), ("4096", "4096")]),   # below 128: the default
    "NLLS_SUPERNODE_PIECE":     ("supernode_piece", [("0", "0"), ("1", "1"), ("5", "5"), ("-1", "-1"), ("x", "0")]),                                 # unset or 0: automatic
    "NLLS_BCR_NT_FULL":         ("bcr_nt_full", [("1", "true"), ("0", "true"), ("", "true")]),
    "NLLS_BCR_LEVEL_BACKWARD":  ("bcr_level_backward", [("1", "true"), ("0", "false"), ("", "false"), ("x", "false")]),
    "NLLS_BCR_CHROWS_SLOTS":    ("bcr_chrows_slots", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0"), ("128", "128")]),
    "NLLS_COST_GRID_MAX":       ("cost_grid_max", [("0", "D"), ("-1", "D"), ("x", "D"), ("1", "1"), ("3", "3"), ("127", "127")]),                    # <= 0 is ignored
    "NLLS_DENSE_DCH1":          ("dense_dch1", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),
    "NLLS_NO_DENSE_WINDOW":     ("no_dense_window", [("1", "true"), ("0", "true"), ("", "true")]),
    "NLLS_NO_TSPARSE":          ("no_tsparse", [("1", "true"), ("0", "true"), ("", "true")]),
    "NLLS_FORCE_TSPARSE":       ("force_tsparse", [("1", "true"), ("0", "true"), ("", "true")]),
    "NLLS_TSP_LEAF":            ("tsp_leaf", [("0", "D"), ("-1", "D"), ("x", "D"), ("1", "1"), ("128", "128")]),
    "NLLS_TSP_CARRY":           ("tsp_carry", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),                                                   # 0 is a value, not "unset"
    "NLLS_TSP_SCHEME":          ("tsp_scheme", [("0", "0"), ("1", "1"), ("3", "3"), ("-1", "-1"), ("x", "0")]),
    "NLLS_TSP_SLOTS":           ("tsp_slots", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),
    "NLLS_TSP_QUAD_MAX":        ("tsp_quad_max", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),
    "NLLS_TSP_CAP":             ("tsp_cap", [("0", "0"), ("1", "1"), ("-1", "-1"), ("x", "0")]),
    "NLLS_TSP_NO_MASKS":        ("tsp_no_masks", [("1", "true"), ("0", "true"), ("", "true")]),
}


def test_every_switch_parses_by_its_own_rule():
    base, table = run(), design_table()
    assert sorted(RULES) == sorted(table)
    for name, (field, cases) in RULES.items():
        assert table[name][0] == field
        for text, want in cases:
            got = run({name: text})
            assert got[field] == (base[field] if want == "D" else want), (name, text, got[field], want)
            assert {k: v for k, v in got.items() if k != field} == {k: v for k, v in base.items() if k != field}, (name, text)      # one switch, one field


def test_an_upload_does_not_read_the_create_time_switches_again():
    table = design_table()
    create = {n: t for n, t in table.items() if t[2] == "create"}
    assert len(create) == 8
    by_hand = dict(spec_on="false", mf_on="false", tiny_dense_on="false", post_fuse="false", elim_split="true", dense_fused_bwd="false", dense_t128_min="-7", singles_wave_min="123456789012")
    assert sorted(by_hand) == sorted(f for f, _, _ in create.values())
    for env in ({}, {n: "1" for n in create}, {n: "0" for n in create}):
        got = run(dict(env, NLLS_TSP_CARRY="0"), "--upload")
        assert {f: got[f] for f in by_hand} == by_hand, env
        assert got["tsp_carry"] == "0"                      # (... while the upload-time ones are read)


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hpp")))


def test_only_the_switches_header_reads_the_environment():
    assert len(_sources()) >= 25
    assert [os.path.basename(f) for f in _sources() if "getenv(" in open(f).read()] == ["nlls_switches.hpp"]


def test_the_header_and_the_design_table_name_the_same_switches():
    assert set(re.findall(r"\bNLLS_[A-Z0-9_]+", open(HDR).read())) == set(design_table())


def test_kernel_attributes_and_the_hip_check_live_in_the_launch_header():
    where = {os.path.basename(f): open(f).read() for f in _sources()}
    assert [f for f, s in where.items() if "hipFuncSetAttribute" in s] == ["nlls_launch.hpp"]
    launch = where["nlls_launch.hpp"]
    body = launch[launch.index("inline hipError_t grant_dynamic_lds("):]
    body = body[:body.index("\n}\n")]
    assert launch.count("hipFuncSetAttribute") == 1 and "hipFuncSetAttribute" in body
    assert sum(s.count("define HIPCHK") for s in where.values()) == 1 and "define HIPCHK" in launch
