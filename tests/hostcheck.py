"""Building the stand-alone host checks (tools/*_hostcheck.cpp: the codecs' core headers under the host compiler and
its sanitizers, each a program of its own that the tests run as a child process)."""
import os
import shutil
import subprocess


def host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "clang++"):
        if cc and shutil.which(cc):
            return cc
    return None


def sanitizers_link(tmp_dir):
    """Whether the host compiler builds and links a trivial program with -fsanitize=address,undefined (a compiler
    without the sanitizer runtimes does not)."""
    if host_compiler() is None:
        return False
    src = os.path.join(tmp_dir, "trivial.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run([host_compiler(), "-fsanitize=address,undefined", src, "-o", os.path.join(tmp_dir, "trivial")],
                       capture_output=True)
    return r.returncode == 0


def build_hostcheck(src, out, sanitize=True):
    """Compile the host check `src` with the host compiler (and the sanitizers) -> out."""
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", src, "-o", out]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    return out
