"""Offsets of the per-node QP record, read from the kernel source (csrc/hsqp_project.h: `constexpr int QP_* = ...;`), so that a test which
slices the raw record follows a layout change instead of silently misaligning."""
import os
import re

from wb_humanoid_mpc_amd import _abi

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wb_humanoid_mpc_amd", "csrc")


def _constants():
    env = {"NX": _abi.NX, "NU": _abi.NU}
    pat = re.compile(r"constexpr int (NUT|QP_[A-Z]+) = ([^;]+);")
    for name in ("hsqp_common.h", "hsqp_project.h"):
        with open(os.path.join(_CSRC, name)) as f:
            for m in pat.finditer(f.read()):
                env[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, env))   # integer arithmetic of the C++ source
    return env


QP = _constants()
NUT = QP["NUT"]
assert QP["QP_A"] == 0 and QP["QP_NUT"] == QP["QP_PE"] + _abi.NU and QP["QP_SIZE"] % 8 == 0, QP
