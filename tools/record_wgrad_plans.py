"""Record how the library runs a weight gradient, per switch state -> tests/golden/wgrad_plans.json.

    python tools/record_wgrad_plans.py [--root TREE] [--only queries|plans]    # rewrite the fixture (or one half of it)
    python tools/record_wgrad_plans.py --child [--root TREE]                   # this process's answers as one JSON line

Two kinds of rows per shape of SHAPES:
  queries  msml_conv_wgrad_workspace, _group_max, _kernel_is_n32, _bnin_applies
  plans    msml_conv_wgrad_plan for the cases of plan_cases(): (status, the eight plan words, slab bytes)
--root names the source tree whose built library answers (default: this one), so the fixture can come from another commit:
the queries from the commit before wgrad_call.h existed, the plans from that commit plus a patch that adds only the plan
query, assembled from that commit's own functions in its own order (a library without the query records no plans).

The file is compact JSON with several rows to a line; a state other than the default keeps only the rows in which it
differs from the default (load_fixture writes them out again).

One fresh child per switch state, with the variable in the CHILD's environment, as tools/record_kernel_names.py does.
Needs no GPU (pure shape queries; msml_num_cus() answers 256 there).  tests/test_wgrad_call_cpu.py replays every state in
one process through _lib.option.  MSML_WGRAD_HALO_NO_REMAP is not recorded: it changes one kernel argument inside the
strip / halo launcher and no answer of these queries."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_plans.json")
F32, BF16 = 0, 1


def cpad(c):                     # ops.cpad: stored channels
    cp = (c + 31) // 32 * 32
    while 64 < cp < 256 and cp & (cp - 1):
        cp += 32
    return cp


def conv(cin, cout, h, r, s, stride, ph, pw, n=256, w=None, btot=None, boff=0, f32=False):
    """Conv2d weight gradient: u = dY [n][p][q][cout], v = X [n][h][w][cin].  -> (shape row, also record f32)"""
    w = h if w is None else w
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    return [cpad(cout), cpad(cin), cout, cin, cin if btot is None else btot, boff, n, h, w, p, q, r, s, stride, ph, pw], f32


def deconv4(cin, cout, p, n=256, q=None, f32=False):
    """ConvTranspose2d(4, 2, 1) weight gradient: u = X on p x q, v = dY on 2p x 2q."""
    q = p if q is None else q
    return [cpad(cin), cpad(cout), cin, cout, cout, 0, n, 2 * p, 2 * q, p, q, 4, 4, 2, 1, 1], f32


def c3(cin, cout, h, n=256, w=None, f32=False):
    return conv(cin, cout, h, 3, 3, 1, 1, 1, n=n, w=w, f32=f32)


def with_a(row, a):              # fewer real rows than stored ones
    row[0][2] = a
    return row


SHAPES = [
    # ---- the workload's layers at batch 256
    c3(64, 64, 112), c3(64, 64, 56, f32=True), c3(128, 128, 28), c3(256, 256, 14, f32=True), c3(512, 512, 7), c3(512, 512, 4, f32=True),
    c3(64, 128, 56), c3(128, 256, 28), c3(256, 512, 14),
    conv(64, 64, 112, 3, 3, 2, 1, 1), conv(128, 128, 56, 3, 3, 2, 1, 1), conv(256, 256, 28, 3, 3, 2, 1, 1),
    conv(512, 512, 14, 3, 3, 2, 1, 1, f32=True),
    conv(64, 64, 112, 1, 1, 2, 0, 0), conv(64, 128, 56, 1, 1, 2, 0, 0, f32=True), conv(128, 256, 28, 1, 1, 2, 0, 0),
    conv(256, 512, 14, 1, 1, 2, 0, 0),
    conv(32, 64, 112, 1, 1, 1, 0, 0),                                   # the im2col'd stem
    conv(512, 512, 7, 7, 7, 1, 0, 0, f32=True),                         # the fc window
    conv(512, 8192, 1, 1, 1, 1, 0, 0), conv(512, 100000, 1, 1, 1, 1, 0, 0),      # PartialFC
    deconv4(18, 18, 56, f32=True), deconv4(18, 18, 28), deconv4(18, 18, 14),     # the OSB deconvs
    c3(32, 32, 56, f32=True), c3(18, 18, 56),
    conv(18, 18, 56, 7, 1, 1, 3, 0, f32=True), conv(18, 18, 56, 1, 7, 1, 0, 3), conv(64, 18, 56, 7, 1, 1, 3, 0),
    conv(64, 18, 56, 1, 7, 1, 0, 3), conv(18, 18, 28, 7, 1, 1, 3, 0), conv(18, 18, 28, 1, 7, 1, 0, 3),
    conv(64, 18, 28, 7, 1, 1, 3, 0), conv(64, 18, 28, 1, 7, 1, 0, 3, f32=True),
    # ---- tests/test_gpu_conv.py: test_conv_wgrad (both dtypes), test_deconv_wgrad
    c3(64, 64, 14, n=3, f32=True), conv(64, 128, 14, 3, 3, 2, 1, 1, n=3, f32=True),
    conv(128, 128, 7, 3, 3, 1, 1, 1, n=3, btot=146, f32=True), conv(18, 128, 7, 3, 3, 1, 1, 1, n=3, btot=146, boff=128, f32=True),
    c3(3, 64, 28, n=3, f32=True), c3(256, 256, 14, n=3, f32=True), conv(64, 128, 14, 1, 1, 2, 0, 0, n=3, f32=True),
    conv(64, 18, 14, 7, 1, 1, 3, 0, n=3, f32=True), conv(512, 512, 7, 7, 7, 1, 0, 0, n=3, f32=True),
    deconv4(36, 18, 7, n=2, f32=True),
    # test_conv_wgrad_halo
    c3(64, 64, 14, n=6), c3(128, 64, 28, n=9), c3(64, 128, 14, n=6), c3(128, 128, 21, n=5, w=28), c3(128, 256, 13, n=4, w=27),
    c3(64, 128, 28, n=40), c3(128, 128, 7, n=7), c3(64, 128, 7, n=10), c3(256, 64, 7, n=33), c3(64, 64, 7, n=1),
    # test_conv_wgrad_group
    c3(256, 256, 14, n=16), c3(128, 128, 28, n=12), c3(64, 64, 56, n=6), c3(128, 64, 21, n=9, w=28), c3(512, 512, 7, n=256),
    c3(256, 256, 7, n=200), c3(128, 128, 7, n=256), c3(512, 512, 4, n=256),
    # test_conv_bn_in_lds_matches_unfused
    c3(128, 128, 28, n=9), c3(128, 256, 28, n=6), c3(256, 256, 14, n=7), c3(256, 128, 13, n=4, w=27),
    # test_conv_wgrad_n32, test_conv_wgrad_line, test_fc_wgrad_window
    deconv4(18, 18, 14, n=3), deconv4(18, 18, 28, n=2), deconv4(18, 18, 15, n=2, q=17), deconv4(18, 18, 56, n=5),
    c3(32, 32, 14, n=3), c3(32, 32, 56, n=2), c3(32, 32, 19, n=2, w=33),
    conv(64, 18, 56, 7, 1, 1, 3, 0, n=4), conv(64, 18, 56, 1, 7, 1, 0, 3, n=4), conv(18, 18, 56, 7, 1, 1, 3, 0, n=4),
    conv(18, 18, 28, 1, 7, 1, 0, 3, n=4), conv(64, 18, 28, 7, 1, 1, 3, 0, n=4),
    conv(512, 512, 7, 7, 7, 1, 0, 0, n=256), conv(64, 96, 7, 7, 7, 1, 0, 0, n=40), conv(32, 32, 4, 4, 4, 1, 0, 0, n=16, btot=96, boff=32),
    conv(64, 64, 3, 3, 3, 1, 0, 0, n=33),
    # tests/test_gpu_wgrad_strip.py
    c3(256, 256, 14, n=17), c3(256, 256, 14, n=5), c3(128, 256, 13, n=12, w=27), c3(128, 128, 21, n=10, w=28), c3(256, 256, 14, n=72),
    # tests/test_gpu_wgrad_plan.py (the smallest shape of every family and variant)
    c3(64, 64, 14, n=2), c3(64, 128, 14, n=2), c3(64, 64, 7, n=5), c3(64, 64, 4, n=8), c3(64, 64, 4, n=64, f32=True),
    c3(128, 128, 4, n=64), conv(64, 64, 8, 1, 1, 1, 0, 0, n=16), c3(32, 32, 14, n=1), deconv4(32, 32, 14, n=1),
    conv(32, 32, 28, 7, 1, 1, 3, 0, n=1), conv(64, 32, 28, 1, 7, 1, 0, 3, n=1), conv(32, 32, 2, 2, 2, 1, 0, 0, n=16),
    # ---- both sides of the predicate edges
    c3(64, 64, 7, n=3), c3(64, 64, 7, n=4),                             # below / above the 70 % rule of the strip kernel
    c3(32, 32, 13, n=8), c3(32, 32, 14, n=8),                           # the narrow-operand kernel's smallest map
    # up = 64 vs 96 STORED channels (written raw: cpad would store 96 channels as 128), on the strip kernel's map and
    # on a small one that goes to the im2col / generic tiles; then fewer real rows than stored ones (A != up), twice
    c3(64, 64, 14, n=8, f32=True), ([96, 64, 96, 64, 64, 0, 8, 14, 14, 14, 14, 3, 3, 1, 1, 1], True),
    ([96, 64, 96, 64, 64, 0, 64, 4, 4, 4, 4, 3, 3, 1, 1, 1], True), ([64, 96, 64, 96, 96, 0, 64, 4, 4, 4, 4, 3, 3, 1, 1, 1], True),
    with_a(c3(64, 64, 14, n=8), 60), c3(64, 96, 14, n=8),
    conv(64, 64, 7, 7, 7, 1, 0, 0, n=16, btot=66, boff=2), conv(64, 64, 7, 7, 7, 1, 0, 0, n=15), conv(64, 64, 7, 7, 7, 1, 0, 0, n=16),
    c3(64, 512, 28, n=2340), c3(64, 512, 28, n=2341),                   # 0x70000000 bytes of dY: strip kernel
    deconv4(18, 18, 112, n=585), deconv4(18, 18, 112, n=586),           # ... of dY: narrow-operand kernel
    conv(64, 64, 8, 1, 1, 1, 0, 0, n=262143), conv(64, 64, 8, 1, 1, 1, 0, 0, n=262144),      # N*P*Q = 2^24 - 64, 2^24
    c3(64, 64, 8, n=262144),
]
SHAPES, WITH_F32 = [r for r, _ in SHAPES], [f for _, f in SHAPES]


def plan_cases():
    """(shape index, dtype, group, bnin): one bf16 layer of every shape, f32 where marked, the 3x3 / stride-1 shapes also in
    groups (2, 3, 4, 8: both sides of every msml_conv_wgrad_group_max) and through the BatchNorm-in-LDS entry point, and
    the refusals of the group entry point."""
    cases = []
    for i, row in enumerate(SHAPES):
        cases.append([i, BF16, 1, 0])
        if WITH_F32[i]:
            cases.append([i, F32, 1, 0])
        if row[11:14] == [3, 3, 1]:
            cases += [[i, BF16, g, 0] for g in (2, 3, 4, 8)] + [[i, BF16, 1, 1]]
    i256, ifc, i1x1 = SHAPES.index(c3(256, 256, 14)[0]), SHAPES.index(conv(512, 512, 7, 7, 7, 1, 0, 0)[0]), \
        SHAPES.index(conv(64, 128, 56, 1, 1, 2, 0, 0)[0])
    cases += [[i256, BF16, 9, 0], [i256, BF16, 0, 0], [i256, F32, 2, 0], [i256, 7, 1, 0], [ifc, BF16, 2, 0], [ifc, BF16, 1, 1],
              [i1x1, BF16, 2, 0], [i1x1, BF16, 1, 1]]
    return cases


# (environment name, text): the parsed value of every one of these is the text as a number ("1" for the presence switches)
STATES = [None, ("MSML_NO_FAST_WGRAD", "1"), ("MSML_NO_FAST_WGRAD_GROUP", "1"), ("MSML_WGRAD_NO_MULTITAP", "1"),
          ("MSML_WGRAD_MULTITAP_WIDE", "0"), ("MSML_WGRAD_WGS", "256"), ("MSML_WGRAD_MINCHUNK", "1024"),
          ("MSML_NO_HALO_WGRAD", "1"), ("MSML_WGRAD_HALO_WIDE_MIN", "256"), ("MSML_WGRAD_HALO_NO_PAIR7", "1"),
          ("MSML_NO_N32_WGRAD", "1"), ("MSML_NO_FC_WGRAD", "1")]


def state_key(state):
    return "default" if state is None else "%s=%s" % state


def answers(root=ROOT):
    """What the library of `root`, loaded in THIS process, answers: {"queries": [...], "plans": [...] or None}."""
    sys.path.insert(0, root)
    from msml_amd import _lib
    lib = _lib.load()
    queries = []
    for up, vp, a, breal, btot, boff, n, h, w, p, q, r, s, stride, ph, pw in SHAPES:
        tail = (n, h, w, p, q, r, s, stride, ph, pw)
        queries.append([lib.msml_conv_wgrad_workspace(up, vp, n, p, q, r, s), lib.msml_conv_wgrad_group_max(up, vp, a, breal, *tail),
                        lib.msml_conv_wgrad_kernel_is_n32(up, vp, *tail), lib.msml_conv_wgrad_bnin_applies(up, vp, a, breal, *tail)])
    if not hasattr(lib, "msml_conv_wgrad_plan"):
        return {"queries": queries, "plans": None}
    plans = []
    for i, dtype, group, bnin in plan_cases():
        words, slab = (ctypes.c_int * 8)(), ctypes.c_long()
        rc = lib.msml_conv_wgrad_plan(*SHAPES[i], dtype, group, bnin, words, ctypes.byref(slab))
        plans.append([rc] + list(words) + [slab.value])
    return {"queries": queries, "plans": plans}


def child_answers(state, root=ROOT):
    """The answers of a fresh process whose environment holds `state` and no other MSML_* variable."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSML_")}
    if state is not None:
        env[state[0]] = state[1]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], env=env, check=True,
                       capture_output=True, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def load_fixture(path=FIXTURE):
    """The fixture with every state written out: on disk a state other than "default" holds only the rows in which it
    differs from the default, as [row index, row]."""
    fixture = json.load(open(path))
    base = fixture["states"]["default"]
    for key, state in fixture["states"].items():
        if key != "default":
            for half, delta in state.items():
                rows = [list(r) for r in base[half]]
                for i, row in delta:
                    rows[i] = row
                state[half] = rows
    return fixture


def save_fixture(fixture, path=FIXTURE, width=118):
    """Compact JSON, several rows to a line."""
    def rows_text(rows):
        lines, line = [], ""
        for r in rows:
            item = json.dumps(r, separators=(",", ":"))
            if line and len(line) + 1 + len(item) > width:
                lines.append(line + ",")
                line = item
            else:
                line = line + "," + item if line else item
        return "[\n" + "\n".join(lines + [line]) + "\n]"
    base = fixture["states"]["default"]
    parts = ['"shapes":' + rows_text(fixture["shapes"]), '"plan_cases":' + rows_text(fixture["plan_cases"])]
    states = []
    for key, state in fixture["states"].items():
        halves = []
        for half, rows in state.items():
            if key != "default":
                rows = [[i, r] for i, (r, b) in enumerate(zip(rows, base[half])) if r != b]
            halves.append('"%s":%s' % (half, rows_text(rows)))
        states.append('"%s":{%s}' % (key, ",\n".join(halves)))
    parts.append('"states":{\n' + ",\n".join(states) + "}")
    with open(path, "w") as f:
        f.write("{" + ",\n".join(parts) + "}\n")


def main():
    argv = sys.argv[1:]
    root = os.path.abspath(argv[argv.index("--root") + 1]) if "--root" in argv else ROOT
    only = argv[argv.index("--only") + 1] if "--only" in argv else None
    if "--child" in argv:
        print(json.dumps(answers(root)))
        return
    fixture = load_fixture() if only and os.path.exists(FIXTURE) else {}
    fixture.update({"shapes": SHAPES, "plan_cases": plan_cases()})
    states = fixture.setdefault("states", {})
    for s in STATES:
        got = child_answers(s, root)
        for half in ("queries", "plans"):
            if only in (None, half):
                assert got[half] is not None, "the library of %s has no msml_conv_wgrad_plan" % root
                states.setdefault(state_key(s), {})[half] = got[half]
    save_fixture(fixture)
    base = states["default"]
    for k, v in states.items():
        print("%-30s differs from the default in %d query rows, %d plan rows" % (
            k, sum(a != b for a, b in zip(v["queries"], base["queries"])),
            sum(a != b for a, b in zip(v.get("plans", []), base.get("plans", [])))))


if __name__ == "__main__":
    main()
