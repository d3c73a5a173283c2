"""One-off: the host-only entry points of two builds, side by side.  Usage:
    python compare_host_calls.py PARENT_LIB_DIR NEW_LIB_DIR
Loads libdeva_hip.so, libdeva_metrics.so and libdeva_vos_metrics.so of both directories with ctypes and calls the
functions that touch no device over the product of the boundary values of tests/*_plan_sanitize_main.cpp.  Every return
value, every plan struct and every *_last_error text must be equal; prints the number of calls compared."""
import ctypes
import itertools
import os
import sys
from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_uint32

I_MIN, I_MAX = -2**31, 2**31 - 1
INF, NAN = float('inf'), float('nan')


class MetricsPlan(ctypes.Structure):
    _fields_ = [('path', c_int32), ('grid', c_uint32), ('block', c_uint32), ('lds_bytes', c_uint32)]


class VosPlan(ctypes.Structure):
    _fields_ = [('label_grid', c_uint32), ('match_grid', c_uint32), ('block', c_uint32), ('lds_bytes', c_uint32),
                ('inner_radius', c_int32), ('radius', c_int32), ('scratch_bytes', c_int64)]


def fields(s):
    return tuple(getattr(s, f[0]) for f in s._fields_)


def load(directory, name, error):
    lib = ctypes.CDLL(os.path.join(os.path.abspath(directory), name))
    if error:
        getattr(lib, error).restype = c_char_p
    return lib


def compare(parent, new, error, calls):
    """calls: (function name, restype, argtypes, argument tuples, out) with out None or a struct / scalar type passed last by
    reference (a None in its place is tried too)"""
    n = 0
    for name, res, argtypes, arguments, out in calls:
        for lib in (parent, new):
            getattr(lib, name).restype = res
            getattr(lib, name).argtypes = argtypes + ([ctypes.c_void_p] if out else [])
        for args in arguments:
            for with_out in ((True, False) if out else (None,)):
                got = []
                for lib in (parent, new):
                    o = out() if with_out else None
                    extra = () if out is None else ((ctypes.addressof(o),) if with_out else (None,))
                    rc = getattr(lib, name)(*args, *extra)
                    value = None if not with_out else (fields(o) if isinstance(o, ctypes.Structure) else o.value)
                    got.append((rc, value if rc == 0 else None, getattr(lib, error)() if error else None))
                assert got[0] == got[1], (name, args, with_out, got)
                n += 1
    return n


def main(parent_dir, new_dir):
    total = 0
    det_counts = [-1, 0, 1, 2, 255, 256, 257, 1024, 1025, 4095, 4096, 4097, 1 << 30]
    det_sides = [-1, 0, 1, 3, 16, 127, 128, 1080, 1920, 46340, 46341, 65536, I_MAX]
    caps = [-1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 1 << 30, I_MAX]
    prompt_sides = [I_MIN, -1, 0, 1, 15, 16, 17, 31, 32, 33, 96, 853, 1080, 1920, 16384, 32768, 32769, 46341, 65535, 65536,
                    65537, 1 << 30, I_MAX]
    prompt_counts = [I_MIN, -1, 0, 1, 9, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 1 << 30, I_MAX]
    rle_sides = [I_MIN, -1, 0, 1, 2, 63, 64, 65, 480, 854, 1080, 1920, 32767, 32768, 32769, 46341, I_MAX]
    rle_channels = [I_MIN, -1, 0, 1, 2, 64, 255, 256, 257, 1023, 1024, 1025, 32767, 32768, I_MAX]
    hip = [load(d, 'libdeva_hip.so', 'deva_hip_last_error') for d in (parent_dir, new_dir)]
    total += compare(*hip, 'deva_hip_last_error', [
        ('deva_detection_scratch', c_int64, [c_int] * 5, itertools.product(det_counts, det_sides, det_sides, det_sides, det_sides), None),
        ('deva_proposal_scratch', c_int64, [c_int], [(c,) for c in caps], None),
        ('deva_prompt_scratch', c_int64, [c_int] * 3, itertools.product(prompt_sides, prompt_sides, prompt_counts), None),
        ('deva_mask_rle_scratch', c_int64, [c_int] * 3, itertools.product(rle_sides, rle_sides, rle_channels), None),
    ])
    pan_sides = [I_MIN, -1, 0, 1, 2, 3, 7, 13, 15, 16, 17, 47, 255, 256, 257, 720, 1080, 1280, 1920, 4095, 4096, 4097, 32767,
                 32768, 32769, 46341, 65536, 1 << 30, (1 << 30) + 1, I_MAX]
    pan_ids = [I_MIN, -1, 0, 1, 2, 40, 100, 125, 126, 127, 253, 254, 255, 510, 1021, 1022, 1023, I_MAX]
    metrics = [load(d, 'libdeva_metrics.so', 'deva_metrics_last_error') for d in (parent_dir, new_dir)]
    total += compare(*metrics, 'deva_metrics_last_error', [
        ('deva_metrics_panoptic_plan', c_int, [c_int] * 4, itertools.product(pan_sides, pan_sides, pan_ids, pan_ids), MetricsPlan),
    ])
    vos_sides = [I_MIN, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 480, 854, 1080, 1920, 4095, 4096, 32767, 32768,
                 32769, 46341, 65536, 1 << 30, (1 << 30) + 1, I_MAX]
    objects = [I_MIN, -1, 0, 1, 2, 5, 63, 64, 65, I_MAX]
    radii = [I_MIN, -1, 0, 1, 2, 3, 4, 8, 36, 127, 128, 129, I_MAX]
    ths = [-INF, -1.0, -1e-300, 0.0, 1e-300, 0.001, 0.008, 0.5, 0.999999, 1.0, 1.5, 2.0, 8.0, 128.0, 128.5, 129.0, 1e18, INF, NAN]
    vos = [load(d, 'libdeva_vos_metrics.so', 'deva_vos_last_error') for d in (parent_dir, new_dir)]
    total += compare(*vos, 'deva_vos_last_error', [
        ('deva_vos_boundary_plan', c_int, [c_int] * 4, itertools.product(vos_sides, vos_sides, objects, radii), VosPlan),
        ('deva_vos_boundary_radius', c_int, [c_int, c_int, c_double], itertools.product(vos_sides, vos_sides, ths), c_int),
        ('deva_vos_boundary_scratch_bytes', c_int, [c_int, c_int], itertools.product(vos_sides, vos_sides), c_int64),
    ])
    print(f'{total} calls compared: every return value, plan and error text equal')


if __name__ == '__main__':
    main(*sys.argv[1:3])
