"""The CPU test bed of the wavefront-emulated kernel tests (tests/test_host_*.py): a kernel's .hip source is compiled for the host through
tests/hostshim_wave64/ (lanes as fibers, collectives as rendezvous points) by a harness tests/host_*_harness.cpp, either into a stand-alone program
`<program> <input file> <results file>` (tests/host_program.h) or into a shared library the test drives through ctypes.  One flag line, one way to run a
program, one way to run it under the host sanitizers: a stand-alone program built with ASan + UBSan and started directly."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PARAMS = os.path.join(REPO, "rtlsdr-airband_amd", "csrc", "params.cpp")  # the plan builder, for the harnesses that run build_plan()
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-DAB_WAVE64_EMU", "-I" + os.path.join(HERE, "hostshim_wave64"), "-I" + os.path.join(REPO, "include")]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_stack_use_after_return=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def build(source, out, *, shared=False, sanitize=False, extra=()):
    """source: a file of tests/, or a list of files (those of other directories with their paths).  extra: what this harness needs beyond FLAGS; it comes
    after them, so an -O level in it holds.  Skips the test where the image has no host clang++.  Returns out."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    sources = [os.path.join(HERE, s) for s in ([source] if isinstance(source, str) else source)]
    cmd = [CLANG] + FLAGS + (["-fPIC", "-shared"] if shared else []) + (SANITIZE if sanitize else []) + list(extra) + ["-o", str(out)] + sources
    subprocess.run(cmd, check=True)
    return str(out)


class Program:
    """A stand-alone harness, built.  dir: where its files go; exe: the program."""

    def __init__(self, directory, name, source, sanitize=False, **kw):
        self.dir, self.name, self.source, self.kw, self.sanitize = str(directory), name, source, kw, sanitize
        self.exe = build(source, os.path.join(self.dir, name + ("_san" if sanitize else "")), sanitize=sanitize, **kw)
        self._twin = None

    def run(self, blob, name):
        """the program on an input file holding blob: (the results file's bytes, what it printed).  Under the sanitizers neither may have reported."""
        src, dst = os.path.join(self.dir, name + ".input"), os.path.join(self.dir, name + ".results")
        with open(src, "wb") as f:
            f.write(blob)
        r = subprocess.run([self.exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **SANITIZER_ENV) if self.sanitize else None)
        assert r.returncode == 0, r.stdout[-4000:]
        if self.sanitize:
            assert "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
        with open(dst, "rb") as f:
            return f.read(), r.stdout

    def sanitized(self):
        """the same source built with -fsanitize=address,undefined, once: its run() asserts that the log holds no report"""
        if self._twin is None:
            self._twin = Program(self.dir, self.name, self.source, sanitize=True, **self.kw)
        return self._twin


def program(tmp_path_factory, name, source, **kw):
    """for a module-scoped fixture: tests/<source> built into a temporary directory of its own"""
    return Program(tmp_path_factory.mktemp(name), name, source, **kw)
