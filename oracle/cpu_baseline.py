"""TEST INFRASTRUCTURE: builds (on the machine it runs on: g++ -O3 -march=native -fopenmp) and drives oracle/cpu_baseline.cpp, the
timed CPU baseline of bench.py.  Only tests/ and bench.py's cpu_baseline leg import this."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "cpu_baseline.cpp")
LIB = os.path.join(_HERE, "_native", "libcpu_baseline.so")     # built per machine (-march=native), never shipped (git-ignored)
FLAGS = ["-O3", "-march=native", "-std=c++17", "-fPIC", "-fopenmp", "-Wno-unknown-pragmas", "-shared"]
_dp = C.POINTER(C.c_double)


def _writable(d):
    try:
        os.makedirs(d, exist_ok=True)
    except OSError:
        return False
    return os.access(d, os.W_OK | os.X_OK)


def _lib_path(deps):
    """oracle/_native/ where the tree is writable; else (a read-only checkout) a private per-user directory under the system
    temp directory, the file named by a hash of the sources, flags and CPU so that no other build is ever picked up."""
    if _writable(os.path.dirname(LIB)):
        return LIB
    h = hashlib.sha256(" ".join(FLAGS + [cpu_model()]).encode())
    for d in deps:
        with open(d, "rb") as f:
            h.update(f.read())
    cache = os.path.join(tempfile.gettempdir(), f"hsqp_cpu_baseline_{os.getuid()}")
    os.makedirs(cache, mode=0o700, exist_ok=True)
    if os.stat(cache).st_uid != os.getuid() or not os.access(cache, os.W_OK | os.X_OK):
        raise RuntimeError(f"{cache} is not a private writable directory: cannot build the CPU baseline")
    return os.path.join(cache, f"libcpu_baseline_{h.hexdigest()[:16]}.so")


def build(force=False):
    csrc = os.path.join(_HERE, "..", "wb_humanoid_mpc_amd", "csrc")
    deps = [SRC] + sorted(os.path.join(csrc, f) for f in os.listdir(csrc))
    lib = _lib_path(deps)
    if force or not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        tmp = f"{lib}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", *FLAGS, SRC, "-o", tmp])
        os.replace(tmp, lib)     # concurrent builders never load a half-written file
    return lib


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """Hardware threads this process may actually use: the affinity mask, capped by the cgroup CPU quota (a container with
    `cpu.max = 1600000 100000` gets 16 CPUs' worth of time however many threads os.cpu_count() reports)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(period)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, period = float(f.read()), float(g.read())
                if q > 0:
                    quota = q / period
        except (OSError, ValueError):
            pass
    return max(1, min(n, int(quota + 0.5))) if quota else n, n, quota


def physical_cores():
    """Distinct (package, core) pairs of /proc/cpuinfo among the CPUs this process may run on: SMT siblings count once."""
    try:
        allowed = os.sched_getaffinity(0)
        seen, cpu, pkg = set(), None, None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k = k.strip()
            if k == "processor":
                cpu = int(v)
            elif k == "physical id":
                pkg = int(v)
            elif k == "core id" and cpu in allowed:
                seen.add((pkg, int(v)))
        return len(seen) or None
    except (OSError, ValueError):
        return None


class CpuBaseline:
    def __init__(self, model):
        self.lib = C.CDLL(build())
        self.lib.cpub_create.restype = C.c_void_p
        self.h = C.c_void_p(self.lib.cpub_create(C.byref(model.desc)))
        if not self.h.value:
            raise RuntimeError("cpub_create failed")

    def __del__(self):
        try:
            self.lib.cpub_destroy(self.h)
        except Exception:
            pass

    def iterate(self, x_init, x, u, par, dt, outer=1, inner=1, iterations=1):
        """(dx[B,N+1,58], du[B,N,35], perf[B,6] = cost, dyn, eq before / after) of the last of `iterations` iterations."""
        x_init, x, u, par = (np.ascontiguousarray(a, dtype=np.float64) for a in (x_init, x, u, par))
        B, N = u.shape[0], u.shape[1]
        dx, du, perf = np.zeros_like(x), np.zeros_like(u), np.zeros((B, 6))
        rc = self.lib.cpub_iterate(self.h, B, N, C.c_double(dt), x_init.ctypes.data_as(_dp), x.ctypes.data_as(_dp), u.ctypes.data_as(_dp),
                                   par.ctypes.data_as(_dp), int(outer), int(inner), int(iterations), dx.ctypes.data_as(_dp), du.ctypes.data_as(_dp),
                                   perf.ctypes.data_as(_dp))
        if rc != 0:
            raise RuntimeError(f"cpu baseline failed: {rc}")
        return dx, du, perf
