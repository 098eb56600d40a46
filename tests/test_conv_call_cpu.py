"""How a conv call travels through msml_amd/csrc (conv_call.h): one struct instead of positional lists, one header of
prototypes instead of hand re-declarations, no thread-local side channel, one reader of the CU count.  Source checks in
the style of test_options_cpu.py::test_one_reader_of_the_environment.  No GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msml_amd", "csrc")
HEADER = "conv_call.h"
# the host functions that choose a conv kernel (the weight-gradient dispatch has its own header, wgrad_call.h, and its own
# test of the same kind, test_wgrad_call_cpu.py)
CONV_NAME = re.compile(r"msml_(?:conv_(?!wgrad)\w+|deconv4)_(?:dispatch|applies|tiling|persist_shape)|msml_conv_fast_splitk")
# a prototype (ends in ';') or a definition (ends in '{'), at file scope or re-declared inside a function
FUNCTION = re.compile(r"^[ \t]*(?:extern\s+)?(?:static\s+)?(?:bool|int)\s+(msml_\w+)\(([^;{]*)\)\s*([;{])", re.M)


def sources():
    return {os.path.basename(p): open(p, errors="replace").read() for p in sorted(glob.glob(os.path.join(CSRC, "*")))
            if os.path.isfile(p)}


def test_one_struct_one_header_no_side_channel():
    src = sources()
    # No mode travels beside the arguments.  core.hip keeps the two per-thread objects that are not arguments of anything:
    # the text behind msml_last_error and the event of msml_stream_wait_stream, both with internal linkage.
    for name, text in src.items():
        lines = [l.strip() for l in text.splitlines() if "thread_local" in l]
        if name == "core.hip":
            assert len(lines) == 2 and all(l.startswith("static thread_local ") for l in lines), lines
        else:
            assert not lines, (name, lines)
    protos, defs = {}, {}
    for name, text in src.items():
        for m in FUNCTION.finditer(text):
            if CONV_NAME.fullmatch(m.group(1)):
                (protos if m.group(3) == ";" else defs).setdefault(m.group(1), []).append((name, m.group(2)))
    assert len(defs) >= 18                                     # 10 dispatch + 7 predicates + the split-K launch
    assert sorted(protos) == sorted(defs)
    for fn in defs:
        assert [f for f, _ in protos[fn]] == [HEADER], (fn, protos[fn])
        assert len(defs[fn]) == 1 and defs[fn][0][0].endswith(".hip"), (fn, defs[fn])
        for _, args in protos[fn] + defs[fn]:
            if fn != "msml_conv_fast_splitk":                  # (a GEMM, not a conv call: plain arguments)
                assert re.fullmatch(r"const Conv(?:Call|Shape)& \w+", args.strip()), (fn, args)
    assert [n for n, t in src.items() if "hipDeviceAttributeMultiprocessorCount" in t] == ["core.hip"]
