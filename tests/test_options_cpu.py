"""The library's option table (msml_amd/csrc/options.h): one reader of the environment, the defaults and the parse rules
every switch had when its site called getenv itself, msml_set_option == the environment variable for the kernel
selection (tests/golden/conv_kernel_names.json, recorded by tools/record_kernel_names.py on the commit BEFORE the table
existed), and the refusals.  No GPU: shape queries only."""
import ctypes
import glob
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

from msml_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msml_amd", "csrc")
OPTION_FILE = "options.hip"

# Written out, not read from the table: the value of every switch with no MSML_* variable in the environment.
DEFAULTS = {
    "MSML_HALO_M16": 2, "MSML_EW_GRID": 768, "MSML_RED_PPT": 16, "MSML_WGRAD_MINCHUNK": 256,
    "MSML_WGRAD_MULTITAP_WIDE": 128, "MSML_WGRAD_HALO_WIDE_MIN": 128, "MSML_CONV_SMALL_M_WGS": 200,
    "MSML_PW_WGS_PER_CU": 4, "MSML_PW_UPW": 1, "MSML_CONV_BIG_TILE": 0, "MSML_R32_ROWS": 0, "MSML_WGRAD_WGS": 0,
    # on by default
    "MSML_HALO_PERSIST": 1, "MSML_WS_M16": 1, "MSML_BNIN_ACC_PERSIST": 1, "MSML_PW_CONV": 1,
}
DEFAULTS.update({name: 0 for name in (     # present-kind: 1 when the variable exists, whatever its text
    "MSML_NO_FAST_CONV", "MSML_CONV_NO_ONE_STAGE", "MSML_CONV_NO_PARITY", "MSML_CONV_NO_SMALL_M", "MSML_NO_X3_SMALL_M",
    "MSML_NO_HALO_CONV", "MSML_HALO_WIDE_ONLY", "MSML_HALO_NO_ONE_SLAB", "MSML_NO_HALO2_CONV", "MSML_NO_HALO2_MOSAIC",
    "MSML_NO_HALO2_S2", "MSML_NO_HALO2_X3", "MSML_NO_WS_CONV", "MSML_NO_S2R_CONV", "MSML_NO_S2R_STRIDE1",
    "MSML_NO_S2R_X3", "MSML_NO_R32_CONV", "MSML_NO_LINE_CONV", "MSML_NO_D4_CONV", "MSML_NO_FAST_WGRAD",
    "MSML_NO_FAST_WGRAD_GROUP", "MSML_WGRAD_NO_MULTITAP", "MSML_NO_HALO_WGRAD", "MSML_WGRAD_HALO_NO_PAIR7",
    "MSML_WGRAD_HALO_NO_REMAP", "MSML_NO_N32_WGRAD", "MSML_NO_FC_WGRAD", "MSML_NO_STEM_LDS")})


def option_names():
    lib = _lib.load()
    return [lib.msml_option_name(i).decode() for i in itertools.takewhile(lambda i: lib.msml_option_name(i), itertools.count())]


def child(code, env_add):
    """Last stdout line of `python -c code` (JSON) in a fresh process with `env_add` and no other MSML_* variable."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSML_") or k == "MSML_LIB"}
    env.update(env_add)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n%s" % (ROOT, code)], env=env,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


READ_ALL = """
import json
from msml_amd import _lib
lib = _lib.load()
names, i = [], 0
while lib.msml_option_name(i):
    names.append(lib.msml_option_name(i).decode()); i += 1
print(json.dumps({"options": {n: _lib.get_option(n) for n in names}, "rows": _lib.value("msml_bn_stats_rows", 100000, 64)}))
"""


def test_one_reader_of_the_environment():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and os.path.basename(path) != OPTION_FILE:
            assert "getenv" not in open(path, errors="replace").read(), path
    assert "getenv" in open(os.path.join(CSRC, OPTION_FILE)).read()
    names = option_names()
    assert len(names) == len(set(names)) and names
    assert sorted(names) == sorted(DEFAULTS)
    assert _lib.load().msml_option_name(len(names)) is None and _lib.load().msml_option_name(-1) is None


def test_every_option_is_in_the_readme_table():
    rows = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("| `MSML_")]
    documented = set()
    for m in re.finditer(r"MSML_\w*(?:\{[\w,]+\}\w*)?", "\n".join(rows)):
        brace = re.match(r"(\w*)\{([\w,]+)\}(\w*)", m.group(0))      # MSML_NO_{HALO,WS}_CONV -> both names
        documented |= {brace.group(1) + x + brace.group(3) for x in brace.group(2).split(",")} if brace else {m.group(0)}
    assert set(option_names()) - documented == set()


def test_defaults_with_an_empty_environment():
    got = child(READ_ALL, {})
    assert got["options"] == DEFAULTS
    assert got["rows"] == 196


def test_legacy_parsing_of_the_environment():
    """The rules of the former per-site reads: presence ("=0" still switches), atoi / atol, "on unless it parses to 0", and
    MSML_PW_CONV's first character; one consumer (the statistics rows: MSML_RED_PPT pixels per thread) sees its value."""
    got = child(READ_ALL, {"MSML_NO_R32_CONV": "0", "MSML_HALO_M16": "1", "MSML_PW_CONV": "all", "MSML_HALO_PERSIST": "0",
                           "MSML_WS_M16": "0", "MSML_RED_PPT": "32"})
    o = got["options"]
    assert [o["MSML_NO_R32_CONV"], o["MSML_HALO_M16"], o["MSML_PW_CONV"], o["MSML_HALO_PERSIST"], o["MSML_WS_M16"],
            o["MSML_RED_PPT"]] == [1, 1, 1, 0, 0, 32]
    assert got["rows"] == 98
    changed = {"MSML_NO_R32_CONV", "MSML_HALO_M16", "MSML_HALO_PERSIST", "MSML_WS_M16", "MSML_RED_PPT"}
    assert {k: v for k, v in o.items() if k not in changed} == {k: v for k, v in DEFAULTS.items() if k not in changed}
    o = child(READ_ALL, {"MSML_PW_CONV": "0", "MSML_NO_FAST_CONV": "", "MSML_BNIN_ACC_PERSIST": "x"})["options"]
    assert [o["MSML_PW_CONV"], o["MSML_NO_FAST_CONV"], o["MSML_BNIN_ACC_PERSIST"]] == [0, 1, 0]     # (atoi("x") == 0)


def answers(queries):
    out = []
    for q in queries:
        v = _lib.value(q[0], *q[1:])
        out.append(v.decode() if isinstance(v, bytes) else v)
    return out


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.load(open(os.path.join(golden_dir, "conv_kernel_names.json")))


def test_selection_unchanged_and_set_option_equals_the_environment(recorded):
    """Every recorded switch state, replayed in THIS process through _lib.option, selects what the variable in a fresh
    process's environment selected before the table existed."""
    queries, states = recorded["queries"], recorded["states"]
    assert len(states) == 15 and len(queries) == 40
    before = {n: _lib.get_option(n) for n in option_names()}
    assert answers(queries) == states["default"]
    for key, want in states.items():
        if key == "default":
            continue
        name, text = key.split("=")
        assert want != states["default"], key          # every recorded state changes at least one answer
        with _lib.option(name, int(text)):
            assert _lib.get_option(name) == int(text)
            got = answers(queries)
        assert got == want, (key, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w])
    assert {n: _lib.get_option(n) for n in option_names()} == before
    assert answers(queries) == states["default"]
    # the example of the issue: msml_conv2d_bnin_acc_applies on 128 -> 128 @ 28x28
    i = queries.index(["msml_conv2d_bnin_acc_applies", 128, 128, 256, 28, 28, 28, 28, 3, 3, 1, 1, 1])
    assert states["default"][i] == 3
    assert {k: states[k][i] for k in ("MSML_HALO_PERSIST=0", "MSML_HALO_M16=1", "MSML_BNIN_ACC_PERSIST=0")} == \
        {"MSML_HALO_PERSIST=0": 1, "MSML_HALO_M16=1": 1, "MSML_BNIN_ACC_PERSIST=0": 1}
    assert [states[k][i] for k in ("MSML_NO_FAST_CONV=1", "MSML_NO_HALO_CONV=1", "MSML_HALO_WIDE_ONLY=1")] == [0, 0, 0]


def test_one_state_through_the_environment_of_a_child(recorded):
    """The start-up path: the recorder's own child mode with the variable in the environment."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSML_") or k == "MSML_LIB"}
    env["MSML_NO_HALO2_CONV"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_kernel_names.py"), "--child"], env=env,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == recorded["states"]["MSML_NO_HALO2_CONV=1"]


def test_refusals():
    lib = _lib.load()
    v = ctypes.c_long(7)
    assert lib.msml_set_option(b"MSML_NO_SUCH_SWITCH", 1) == _lib.UNSUPPORTED
    assert b"MSML_NO_SUCH_SWITCH" in lib.msml_last_error()
    assert lib.msml_get_option(b"MSML_NO_SUCH_SWITCH", ctypes.byref(v)) == _lib.UNSUPPORTED and v.value == 7
    assert b"MSML_NO_SUCH_SWITCH" in lib.msml_last_error()
    assert lib.msml_set_option(None, 1) == -1                      # MSML_ERR_SHAPE
    assert lib.msml_get_option(None, ctypes.byref(v)) == -1
    assert lib.msml_get_option(b"MSML_HALO_M16", None) == -1
    with pytest.raises(KeyError):
        _lib.set_option("MSML_NO_SUCH_SWITCH", 1)
    with pytest.raises(KeyError):
        _lib.get_option("MSML_NO_SUCH_SWITCH")
    with pytest.raises(KeyError):
        with _lib.option("MSML_NO_SUCH_SWITCH", 1):
            pass
