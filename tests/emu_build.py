"""Test helper: how the host emulations under tests/emu are compiled.  The emu_*_driver modules name their sources and headers and
call shared() for the library they load and program() for the stand-alone program the sanitizers run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas"]


def deps(*sources, headers=()):
    """The files a build depends on: sources under tests/emu, headers under csrc, and what every emulation includes."""
    csrc = os.path.join(HERE, "..", "topsicle_amd", "csrc")
    return [os.path.join(EMU, s) for s in sources + ("emu_batch.h",)] + [os.path.join(csrc, h) for h in tuple(headers) + ("tps_check.h",)] + \
           [os.path.join(HERE, "..", "include", "topsicle_hip.h")]


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def _compile(cmd, out):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp%d" % os.getpid()
    subprocess.check_call(cmd + ["-o", tmp])
    os.replace(tmp, out)
    return out


def shared(name, src, deps, asan=False):
    """tests/emu/<src> as the shared object tests/emu/_build/<name>, for ctypes; asan: under -fsanitize=address,undefined (at -O1:
    -O2 -g takes three times as long to compile)."""
    out = os.path.join(EMU, "_build", name)
    if _fresh(out, deps):
        return out
    san = ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if asan else []
    return _compile(["g++", "-O2"] + FLAGS + ["-shared", "-fPIC"] + san + [os.path.join(EMU, src)], out)


def program(name, main_src, deps):
    """tests/emu/<main_src> as the stand-alone program tests/emu/_build/<name> (its own main, nothing loaded into Python) under
    -fsanitize=address,undefined."""
    out = os.path.join(EMU, "_build", name)
    if _fresh(out, deps + [os.path.join(EMU, main_src)]):
        return out
    return _compile(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS +
                    [os.path.join(EMU, main_src)], out)
