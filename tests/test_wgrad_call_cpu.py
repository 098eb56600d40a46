"""How a weight-gradient call travels through msml_amd/csrc (wgrad_call.h): one struct instead of positional lists, one
header of prototypes instead of hand re-declarations, one plan; and the selection it makes, per switch state, against
tests/golden/wgrad_plans.json (recorded by tools/record_wgrad_plans.py on the commit BEFORE the header existed).
Source checks in the style of test_conv_call_cpu.py.  No GPU: shape queries only."""
import ctypes
import glob
import json
import os
import re

import pytest

from msml_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msml_amd", "csrc")
HEADER = "wgrad_call.h"
WGRAD_NAME = re.compile(r"msml_(?:fc_)?wgrad_\w+")
# a prototype (ends in ';') or a definition (ends in '{'), at file scope or re-declared inside a function
FUNCTION = re.compile(r"^[ \t]*(?:extern\s+)?(?:static\s+)?(?:bool|int|void|long)\s+(msml_\w+)\(([^;{]*)\)\s*([;{])", re.M)
ARG = re.compile(r"const Wgrad(?:Shape|Call|Plan)&(?: \w+)?|int \w+")
FAMILY, VARIANT, BA, BB, NTW, SPLITS, CHUNK, DIRECT = range(8)      # the words of msml_conv_wgrad_plan
FC, N32, LINE, HALO, FAST, GENERIC = range(1, 7)


def sources():
    return {os.path.basename(p): open(p, errors="replace").read() for p in sorted(glob.glob(os.path.join(CSRC, "*")))
            if os.path.isfile(p)}


def test_one_struct_one_header_one_plan():
    src = sources()
    protos, defs = {}, {}
    for name, text in src.items():
        for m in FUNCTION.finditer(text):
            if WGRAD_NAME.fullmatch(m.group(1)):
                (protos if m.group(3) == ";" else defs).setdefault(m.group(1), []).append((name, m.group(2)))
    assert len(defs) >= 14                                     # 9 predicates + 5 launchers
    assert sorted(protos) == sorted(defs)
    for fn in defs:
        assert [f for f, _ in protos[fn]] == [HEADER], (fn, protos[fn])
        assert len(defs[fn]) == 1 and defs[fn][0][0].endswith(".hip"), (fn, defs[fn])
        for _, args in protos[fn] + defs[fn]:
            args = [a.strip() for a in args.split(",")]
            assert all(ARG.fullmatch(a) for a in args), (fn, args)
            assert args[0].startswith("const WgradShape&") or args[0].startswith("const WgradCall&"), (fn, args)
            assert sum(a.startswith("int ") for a in args) <= 1, (fn, args)
    # no .hip file declares a function of another file: every prototype of a host function sits in a header
    for name, text in src.items():
        if name.endswith(".hip"):
            own = {m.group(1) for m in FUNCTION.finditer(text) if m.group(3) == "{"}
            foreign = [m.group(1) for m in FUNCTION.finditer(text) if m.group(3) == ";" and m.group(1) not in own]
            if name in ("conv_wgrad.hip", "wgrad_fast.hip", "wgrad_halo.hip", "wgrad_n32.hip", "fc_wgrad.hip"):
                assert not foreign, (name, foreign)
    # the split rule and the taps-per-workgroup rule are reached from one function
    text = src["conv_wgrad.hip"]
    bodies = re.split(r"^(?=(?:static|extern \"C\")\s)", text, flags=re.M)
    for rule in ("pick_splits", "wgrad_ntw", "pick_tile"):
        callers = [b.split("(")[0] for b in bodies if re.search(r"\b%s\(" % rule, b) and not re.match(r"static int %s\(" % rule, b)]
        assert len(callers) == 1 and callers[0].endswith("wgrad_tile_plan"), (rule, callers)
        assert all(rule + "(" not in t for n, t in src.items() if n != "conv_wgrad.hip"), rule
    for gone in ("WR_MAXGROUP", "WF_MAXGROUP", "WH_MAXGROUP"):
        assert all(gone not in t for t in src.values()), gone


def plan(shape, dtype, group, bnin):
    words, slab = (ctypes.c_int * 8)(), ctypes.c_long()
    rc = _lib.load().msml_conv_wgrad_plan(*shape, dtype, group, bnin, words, ctypes.byref(slab))
    return [rc] + list(words) + [slab.value]


def answers(recorded):
    lib = _lib.load()
    queries = []
    for up, vp, a, breal, btot, boff, n, h, w, p, q, r, s, stride, ph, pw in recorded["shapes"]:
        tail = (n, h, w, p, q, r, s, stride, ph, pw)
        queries.append([lib.msml_conv_wgrad_workspace(up, vp, n, p, q, r, s), lib.msml_conv_wgrad_group_max(up, vp, a, breal, *tail),
                        lib.msml_conv_wgrad_kernel_is_n32(up, vp, *tail), lib.msml_conv_wgrad_bnin_applies(up, vp, a, breal, *tail)])
    return queries, [plan(recorded["shapes"][i], dtype, group, bnin) for i, dtype, group, bnin in recorded["plan_cases"]]


@pytest.fixture(scope="module")
def recorded(golden_dir):
    """The fixture with every state written out: the file keeps, for a state other than the default, only the rows in which
    it differs from the default, as [row index, row]."""
    fixture = json.load(open(os.path.join(golden_dir, "wgrad_plans.json")))
    base = fixture["states"]["default"]
    for key, state in fixture["states"].items():
        for half in ("queries", "plans") if key != "default" else ():
            rows = [list(r) for r in base[half]]
            for i, row in state[half]:
                assert rows[i] != row, (key, half, i)
                rows[i] = row
            state[half] = rows
    return fixture


def check_rows_agree(recorded, queries, plans, key):
    """The four older queries are readers of the same plan, and no plan writes more than the workspace query grants."""
    cases = recorded["plan_cases"]
    for i, (ws, gmax, is_n32, bnin_applies) in enumerate(queries):
        one = plans[cases.index([i, _lib.BF16, 1, 0])]
        assert is_n32 == int(one[1 + FAMILY] in (N32, LINE)), (key, i)
        if [i, _lib.BF16, 1, 1] in cases:
            bn = plans[cases.index([i, _lib.BF16, 1, 1])]
            assert bnin_applies == int(bn[0] == 0), (key, i)
            assert bn[0] != 0 or (bn[1 + FAMILY] == HALO and bn[1 + VARIANT] in (64, 128)), (key, i, bn)
        else:
            assert bnin_applies == 0, (key, i)
    for (i, dtype, group, bnin), row in zip(cases, plans):
        if row[0] == 0:
            up, vp, taps = recorded["shapes"][i][0], recorded["shapes"][i][1], recorded["shapes"][i][11] * recorded["shapes"][i][12]
            assert row[-1] <= queries[i][0], (key, i, row)
            assert row[-1] == (0 if row[1 + DIRECT] else group * row[1 + SPLITS] * up * taps * vp * 4), (key, i, row)
            # a shape the group query calls groupable keeps, as a group of one, the strip / halo or im2col plan (the group
            # query does not look at MSML_NO_FAST_WGRAD; a group of one now honours it like msml_conv_wgrad)
            if group == 1 and not bnin and dtype == _lib.BF16 and queries[i][1] > 1 and key != "MSML_NO_FAST_WGRAD=1":
                assert row[1 + FAMILY] in (HALO, FAST), (key, i, row)


def test_selection_unchanged_and_set_option_equals_the_environment(recorded):
    """Every recorded switch state, replayed in THIS process through _lib.option, answers what the variable in a fresh
    process's environment made the library answer before wgrad_call.h existed."""
    states = recorded["states"]
    assert len(states) == 12 and len(recorded["shapes"]) >= 100 and len(recorded["plan_cases"]) >= 300
    base = states["default"]
    queries, plans = answers(recorded)
    assert queries == base["queries"]
    assert plans == base["plans"], [(c, g, w) for c, g, w in zip(recorded["plan_cases"], plans, base["plans"]) if g != w][:5]
    check_rows_agree(recorded, queries, plans, "default")
    for key, want in states.items():
        if key == "default":
            continue
        name, text = key.split("=")
        assert want["queries"] != base["queries"] or want["plans"] != base["plans"], key      # every state changes an answer
        with _lib.option(name, int(text)):
            queries, plans = answers(recorded)
        assert queries == want["queries"], (key, [(s, g, w) for s, g, w in zip(recorded["shapes"], queries, want["queries"]) if g != w][:5])
        assert plans == want["plans"], (key, [(c, g, w) for c, g, w in zip(recorded["plan_cases"], plans, want["plans"]) if g != w][:5])
        check_rows_agree(recorded, queries, plans, key)
    assert answers(recorded) == (base["queries"], base["plans"])


def test_every_family_and_refusal_is_recorded(recorded):
    """The fixture reaches what it is meant to pin: every family, the three strip variants, direct tiles, and each status."""
    rows = recorded["states"]["default"]["plans"]
    ok = [r for r in rows if r[0] == 0]
    assert {r[1 + FAMILY] for r in ok} == {FC, N32, LINE, HALO, FAST, GENERIC}
    assert {r[1 + VARIANT] for r in ok if r[1 + FAMILY] == HALO} == {64, 128, 7}
    assert {r[1 + NTW] for r in ok if r[1 + FAMILY] == FAST} == {1, 3}
    assert any(r[1 + DIRECT] and r[1 + FAMILY] == FAST for r in ok)
    assert {r[0] for r in rows} == {0, -1, _lib.UNSUPPORTED, -2}          # ok, shape, unsupported, dtype
    generic_bf16 = [r for r in recorded["states"]["MSML_NO_FAST_WGRAD=1"]["plans"] if r[0] == 0 and r[1 + FAMILY] == GENERIC and r[1 + NTW] == 3]
    assert generic_bf16                                                  # (the generic bf16 launch keeps the fast split count)
