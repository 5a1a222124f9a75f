"""The host build of csrc/norm_plan.h (tests/norm_plan_host.cpp, g++, no GPU) and the Python side of its ABI, shared by
tests/test_norm_plan_host.py, tests/test_norm_cases_host.py and tests/test_norm_kernels_gpu.py.  libkd6d.so is not
loaded here."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LL = ctypes.c_longlong
CONSTANTS = ("threads", "flush_lds", "bn_hold", "pool_hold", "gn_hold", "bn_blocks", "colstats_cap", "bn_reduce_cap",
             "gn_bwd_max_c")


def build_lib(directory):
    so = os.path.join(str(directory), "libnormplan.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "norm_plan_host.cpp")])
    L = ctypes.CDLL(so)
    for n in ("np_flush_lds_bytes", "np_bn_apply_lds_bytes", "np_bn_onepass_lds_bytes", "np_gn_bwd_lds_bytes"):
        getattr(L, n).restype = LL
    for n in ("np_grid_for", "np_bn_bwd_reduce_grid", "np_bn_pool_bwd_reduce_grid"):
        getattr(L, n).argtypes = [LL]
    L.np_colstats_grid.argtypes = [LL, ctypes.c_int]
    L.np_bn_onepass_plan.argtypes = [LL, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, LL, ctypes.POINTER(ctypes.c_int)]
    c = (ctypes.c_int * len(CONSTANTS))()
    L.np_constants(c)
    L.k = dict(zip(CONSTANTS, c))
    return L
