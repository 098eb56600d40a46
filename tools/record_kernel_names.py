"""Record which conv kernel the library selects, per switch state -> tests/golden/conv_kernel_names.json.

    python tools/record_kernel_names.py            # rewrite the fixture
    python tools/record_kernel_names.py --child    # print this process's answers as one JSON list (used above and by the test)

One fresh child per switch state, with the variable in the CHILD's environment: the recording goes through the library's
start-up read of the environment only, so the same script records any commit.  Needs no GPU (pure shape queries).
tests/test_options_cpu.py replays every state in one process through _lib.option and compares with the fixture."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_kernel_names.json")
N, F32, BF16 = 256, 0, 1


def _conv(c0p, c1p, cout, h, p, r, s, stride, ph, pw, transposed, dt=BF16):
    return [c0p, c1p, cout, N, h, h, p, p, r, s, stride, ph, pw, transposed, dt, dt]


def _c3(cin, cout, h):
    return _conv(cin, 0, cout, h, h, 3, 3, 1, 1, 1, 0)


def _s2(c, h, transposed):      # 3x3 stride 2 @ h x h: forward h -> h / 2, transposed (backward-data) h / 2 -> h
    return _conv(c, 0, c, h // 2, h, 3, 3, 2, 1, 1, 1) if transposed else _conv(c, 0, c, h, h // 2, 3, 3, 2, 1, 1, 0)


KERNEL_SHAPES = [
    _c3(256, 256, 14), _c3(128, 128, 28), _c3(64, 128, 56), _c3(64, 64, 56),
    _s2(64, 112, 0), _s2(64, 112, 1), _s2(128, 56, 0), _s2(128, 56, 1),
    _c3(512, 512, 7), _s2(512, 14, 0), _s2(512, 14, 1), _c3(512, 512, 4), _c3(256, 256, 7),
    _conv(64, 0, 32, 56, 56, 7, 1, 1, 3, 0, 0),                 # 7x1 line conv
    _conv(32, 32, 32, 56, 112, 4, 4, 2, 1, 1, 1),               # 4x4 stride-2 transposed on cat(32, 32)
    _conv(64, 0, 128, 56, 56, 1, 1, 1, 0, 0, 0), _conv(32, 0, 32, 56, 56, 1, 1, 1, 0, 0, 0),
    _conv(64, 0, 64, 56, 56, 3, 3, 1, 1, 1, 0, F32),
]
QUERIES = [["msml_conv2d_kernel"] + a + [ws] for a in KERNEL_SHAPES for ws in (0, 1)]
QUERIES += [["msml_conv2d_bnin_acc_applies", cin, cout, N, h, h, h, h, 3, 3, 1, 1, 1]
            for cin, cout, h in ((128, 128, 28), (64, 128, 56), (256, 256, 14))]
QUERIES += [["msml_conv2d_bnin_applies", 256, 256, N, 14, 14, 14, 14, 3, 3, 1, 1, 1, 1]]

# (environment name, text): the parsed value of every one of these is the text as a number ("1" for the presence switches)
STATES = [None, ("MSML_HALO_PERSIST", "0"), ("MSML_HALO_M16", "1"), ("MSML_NO_FAST_CONV", "1"),
          ("MSML_HALO_NO_ONE_SLAB", "1"), ("MSML_NO_HALO_CONV", "1"), ("MSML_HALO_WIDE_ONLY", "1"),
          ("MSML_NO_WS_CONV", "1"), ("MSML_NO_S2R_CONV", "1"), ("MSML_NO_HALO2_S2", "1"), ("MSML_NO_HALO2_MOSAIC", "1"),
          ("MSML_NO_HALO2_CONV", "1"), ("MSML_NO_LINE_CONV", "1"), ("MSML_NO_D4_CONV", "1"),
          ("MSML_BNIN_ACC_PERSIST", "0")]


def state_key(state):
    return "default" if state is None else "%s=%s" % state


def answers(queries=QUERIES):
    """What the library loaded in THIS process answers, in the order of `queries`."""
    sys.path.insert(0, ROOT)
    from msml_amd import _lib
    out = []
    for q in queries:
        v = _lib.value(q[0], *q[1:])
        out.append(v.decode() if isinstance(v, bytes) else v)
    return out


def child_answers(state):
    """The answers of a fresh process whose environment holds `state` and no other MSML_* variable."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSML_") or k == "MSML_LIB"}
    if state is not None:
        env[state[0]] = state[1]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if "--child" in sys.argv:
        print(json.dumps(answers()))
        return
    fixture = {"queries": QUERIES, "states": {state_key(s): child_answers(s) for s in STATES}}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=0, separators=(",", ":"))
        f.write("\n")
    base = fixture["states"]["default"]
    for k, v in fixture["states"].items():
        print("%-26s %d answers differ from the default" % (k, sum(a != b for a, b in zip(v, base))))
    print("kernel names:", len({a for v in fixture["states"].values() for a in v if isinstance(a, str)}))


if __name__ == "__main__":
    main()
