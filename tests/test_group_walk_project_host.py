"""The group walker's delivery side on the CPU under the address and undefined-behaviour sanitizers: csrc/gw_proj.h
(k_gtile_count, k_gscan_project<RPT> and their launches) compiled with SG_HOST_ONLY over tests/host_gwproj/simt_shim.h
(a workgroup is 256 host threads) into a stand-alone program, tests/host_gwproj/harness.cpp, which lays trigger words
and a match area out as the walker does, in buffers of exactly run_group_walk's sizes, runs both kernels for RPT 1, 2
and 4 and compares the records with a serial projection.  Its cases are the densest tile (a list at its bound) and the
trigger that ends the match area (1, 2 and 3 matches: the two entries read with every header), which is where a read
past a buffer would be; no GPU is involved.  The compiler is ROCm's clang++ (the kernels use its vector types and
builtins), which brings the sanitizer runtimes; the program links them, nothing is preloaded."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_gwproj")
BUILD = os.path.join(SRC, "_build")
FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def clangxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
              shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no clang++ (ROCm's lib/llvm/bin/clang++ or one on PATH)")


def build():
    exe = os.path.join(BUILD, "gwproj_san")
    deps = [os.path.join(SRC, "harness.cpp"), os.path.join(SRC, "simt_shim.h"),
            os.path.join(ROOT, "siddhi_amd", "csrc", "gw_proj.h"), os.path.join(ROOT, "include", "siddhi_gpu.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.run([clangxx()] + FLAGS + [deps[0], "-o", tmp], check=True)
        os.replace(tmp, exe)
    return exe


def test_projection_under_sanitizers():
    p = subprocess.run([build()], env=ENV, capture_output=True, text=True, timeout=600)
    report = "ERROR: AddressSanitizer" in p.stderr or "runtime error:" in p.stderr or "LeakSanitizer" in p.stderr
    assert p.returncode == 0 and not report, (p.stdout + p.stderr)[-4000:]
    lines = p.stdout.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["dense", "end_m1", "end_m2", "end_m3"]
    assert all(ln.endswith(" ok") for ln in lines), p.stdout
