"""The host build of csrc/conv_plan.h (tests/conv_plan_host.cpp, g++, no GPU) and the Python side of its ABI, shared by
tests/test_conv_plan_host.py, tests/test_conv_variant_cases_host.py and tests/test_conv_variants_gpu.py.  libkd6d.so is
not loaded here."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

LL = ctypes.c_longlong
NCU = 256
BF16, F32 = 0, 1
SMALLC, HALO, SPLITK, GLDS, IGEMM = range(5)
WG_SMALL, WG_TR, WG_GENERIC = range(3)
CONV_FIELDS = ("family BP BC WP WC NSTAGE HMAX CG NB PDB NORM XF grid_x grid_y threads lds n_ctiles n_ptiles p_fastest nk_split "
               "nsplit finalize_grid halo total_rows patch_bytes wbytes fused_epilogue").split()
WGRAD_FIELDS = "family BN BJ WN WJ CG NB KS parts m_chunk n_jtiles grid_x grid_y lds R tiles_per_img ntiles buf_bytes prow".split()
OPT_NAMES = ("halo", "halo_pairing", "halo_wide", "smallc", "smallc_wmax", "splitk", "tile", "wgrad_small")
OPT_DEFAULT = dict(halo=-1, halo_pairing=1, halo_wide=1, smallc=-1, smallc_wmax=640, splitk=-1, tile=-1, wgrad_small=-1)
WS_BYTES = 64 << 20          # the split-K workspace of tools/bench_conv.py
LISTS = ("igemm", "glds", "splitk", "smallc", "halo", "halo_norm", "wgrad", "wgrad_tr", "wgrad_small")


class Plan(dict):
    __getattr__ = dict.__getitem__


def build_lib(directory):
    so = os.path.join(str(directory), "libconvplan.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "conv_plan_host.cpp")])
    return ctypes.CDLL(so)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


_OPTS = {}


def _opts(o):
    key = tuple(sorted(o.items()))
    if key not in _OPTS:
        _OPTS[key] = _ints([dict(OPT_DEFAULT, **o)[n] for n in OPT_NAMES])
    return _OPTS[key]


class Layer:
    """One convolution over a pyramid of input levels, packed back to back as kd6d.ops.Geom packs them."""

    def __init__(self, batch, cin, cout, k, stride, levels, out_shift=0):
        self.batch, self.cin, self.cout, self.k, self.stride, self.pad = batch, cin, cout, k, stride, k // 2
        self.levels = [tuple(l) for l in levels]
        self.out = [((h + 2 * self.pad - k) // stride + 1, (w + 2 * self.pad - k) // stride + 1) for h, w in self.levels]
        self.seg, rin, rout = [], 0, out_shift
        for (h, w), (ho, wo) in zip(self.levels, self.out):
            self.seg += [h, w, rin, rout]
            rin += batch * h * w
            rout += batch * ho * wo
        self.rows_in, self.rows_out = rin, rout - out_shift
        self.out_hw = [ho * wo for ho, wo in self.out]
        self.wmax = max(w for _, w in self.levels)
        self._shape = {}

    def shape(self, kind):
        kind = "dgrad" if kind == "dgrad" else "fwd"
        if kind not in self._shape:
            self._shape[kind] = self._make_shape(kind)
        return self._shape[kind]

    def _make_shape(self, kind):
        taps = self.k * self.k
        if kind == "dgrad":
            head = [self.rows_in, self.cin, self.cout, taps * self.cout]
        else:
            head = [self.rows_out, self.cout, self.cin, taps * self.cin]
        return _ints(head + [self.k, self.stride, self.pad, self.batch, len(self.levels)] + self.seg)


def plan_conv(lib, layer, kind="fwd", dtype=BF16, stats=0, groups=0, replicas=0, norm=0, xf=0, ws=0, pair=0, ncu=NCU,
              ws_bytes=WS_BYTES, **opts):
    out = (LL * len(CONV_FIELDS))()
    lib.cp_plan_conv(layer.shape(kind), _ints([dtype, stats, groups, replicas, norm, xf, ws, pair]), LL(ws_bytes if ws else 0),
                     _opts(opts), ncu, int(kind == "dgrad"), out)
    return Plan(zip(CONV_FIELDS, out))


def plan_wgrad(lib, layer, dtype=BF16, bias=0, budget=0, ncu=NCU, **opts):
    out = (LL * len(WGRAD_FIELDS))()
    lib.cp_plan_wgrad(layer.shape("wgrad"), dtype, bias, _opts(opts), ncu, budget, out)
    return Plan(zip(WGRAD_FIELDS, out))


def fusable(lib, layer, dtype, kind, groups, fuse_norm=3, pair=0, **opts):
    return lib.cp_norm_fusable(layer.shape("fwd"), _ints(layer.out_hw), dtype, kind, groups, fuse_norm, pair, _opts(opts), NCU)


def stats_table(lib, layer, dtype, groups, norm=0, ncu=NCU, **opts):
    """The group-statistics LDS table of the forward launch planned for the layer (conv_plan.h stats_table_*): room = keys
    per tile the planned kernel holds, tile_keys = the most (level, image) keys any of its tiles touches, fits, bytes, lds."""
    out = (LL * 5)()
    lib.cp_stats_table(layer.shape("fwd"), _ints([dtype, 1, groups, 0, norm, 0, 0, 0]), _opts(opts), ncu, out)
    return Plan(zip("room tile_keys fits bytes lds".split(), out))


def stats_row_key(lib, layer, m):
    """level * batch + image of forward GEMM row m (conv_plan.h stats_row_key, the host form of the kernels' stats_key)."""
    return lib.cp_stats_row_key(layer.shape("fwd"), m)


def variants(lib, name):
    """The rows of the KD6D_CONV_*_TILES list `name` (LISTS), as tuples of 6 ints with the unused columns 0."""
    buf = (ctypes.c_int * (6 * 64))()
    return [tuple(buf[6 * r:6 * r + 6]) for r in range(lib.cp_variants(LISTS.index(name), buf))]
