"""Per-ray records without a GPU: the new symbols, argument checks that come before any HIP call, the Rust-Display float
formatter and the debug CSV of a hand-built RayRecords."""
import ctypes as C
import io

import numpy as np

RTMI_OK, RTMI_ERR_INVALID = 0, 1


class Vp(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi.lib(), _ffi


def test_symbols_exported_and_listed():
    L, ffi = _lib()
    for name in ("rtmi_trace_records", "rtmi_primary_records"):
        assert name in ffi.RTMI_SYMBOLS and hasattr(L, name)
    for name in ("rth_caster_trace_records", "rth_caster_primary_records", "rth_scene_set_debug", "rth_scene_debug_records"):
        assert name in ffi.RTH_SYMBOLS and hasattr(L, name)
    assert C.sizeof(ffi.RayRecord) == 72 and ffi.RayRecord.leaf_first.offset == 48
    from rust_raytrace_amd import raytrace as R
    assert R.REC_DTYPE.itemsize == 72 and R.REC_DTYPE.fields["leaf_first"][1] == 48


def test_invalid_arguments_before_any_hip_call():
    """No device here: a status other than RTMI_ERR_INVALID (or RTMI_OK) would mean the call reached HIP first.  The
    scene handle is an opaque non-NULL pointer the checks must not need."""
    L, ffi = _lib()
    from rust_raytrace_amd import raytrace as R
    fake = C.create_string_buffer(1 << 16)
    o4 = np.zeros((2, 4), np.float32)
    d4 = np.tile(np.array([0, 0, 1, 0], np.float32), (2, 1))
    recs = np.zeros(64, R.REC_DTYPE)
    tot = C.c_uint64(99)
    p = R._p

    def expect(rc, code=RTMI_ERR_INVALID):
        assert rc == code, (rc, L.rtmi_last_error())
        if code != RTMI_OK:
            assert L.rtmi_last_error().decode()

    expect(L.rtmi_trace_records(None, 2, p(o4), p(d4), p(recs), None, 0, C.byref(tot), None))
    expect(L.rtmi_trace_records(fake, 2, p(o4), p(d4), None, None, 0, C.byref(tot), None))
    expect(L.rtmi_trace_records(fake, 2, None, p(d4), p(recs), None, 0, C.byref(tot), None))
    expect(L.rtmi_trace_records(fake, 2, p(o4), p(d4), p(recs), None, 0, None, None))
    expect(L.rtmi_trace_records(fake, 0, None, None, None, None, 0, C.byref(tot), None), RTMI_OK)
    assert tot.value == 0
    vp = Vp(8, 6, (C.c_float * 3)(2, 0, 0), (C.c_float * 3)(2, 0, 1), (C.c_float * 3)(0, 1, 0), (C.c_float * 3)(1, 0, 0), 5, 4)
    expect(L.rtmi_primary_records(None, C.byref(vp), 1, 0, 6, 0, p(recs), None, 0, C.byref(tot), None))
    expect(L.rtmi_primary_records(fake, None, 1, 0, 6, 0, p(recs), None, 0, C.byref(tot), None))
    expect(L.rtmi_primary_records(fake, C.byref(vp), 1, 0, 6, 0, None, None, 0, C.byref(tot), None))
    expect(L.rtmi_primary_records(fake, C.byref(vp), 1, 0, 6, 4, p(recs), None, 0, C.byref(tot), None))  # sample >= spp
    assert "sample" in L.rtmi_last_error().decode()
    expect(L.rtmi_primary_records(fake, C.byref(vp), 1, 2, 5, 0, p(recs), None, 0, C.byref(tot), None))  # rows 2..6 of 6
    assert "row" in L.rtmi_last_error().decode()
    expect(L.rtmi_primary_records(fake, C.byref(vp), 1, 7, 0, 0, p(recs), None, 0, C.byref(tot), None))  # row0 past the frame
    expect(L.rtmi_primary_records(fake, C.byref(vp), 1, 6, 0, 0, None, None, 0, C.byref(tot), None), RTMI_OK)  # nrows == 0


def test_rust_display_float_format():
    from rust_raytrace_amd.raytrace import format_f32
    cases = [(1.0, "1"), (0.1, "0.1"), (1e-10, "0.0000000001"), (-0.0, "-0"), (0.0, "0"), (float("nan"), "NaN"), (float("inf"), "inf"),
             (float("-inf"), "-inf"), (-2.5, "-2.5"), (3.4028235e38, "340282350000000000000000000000000000000"), (0.3, "0.3"),
             (16777216.0, "16777216")]
    for x, want in cases:
        assert format_f32(np.float32(x)) == want, (x, format_f32(np.float32(x)), want)


class _Tree:
    """Scene.tree() of a root with three leaves: box 1 lists (5, 2), box 2 lists (2, 9, 7), box 3 is empty"""

    def tree(self):
        topo = np.array([[1, 3, 0, 0], [0, 2, 1, 1], [2, 3, 1, 1], [5, 0, 1, 1]], np.uint32)
        return np.zeros((4, 4), np.float32), topo, np.array([5, 2, 2, 9, 7], np.uint32)


def test_write_csv_of_hand_built_records():
    from rust_raytrace_amd import raytrace as R
    recs = np.zeros(3, R.REC_DTYPE)
    recs["orig"] = [[2, 0, 0, 0], [0.1, -0.0, 1e-10, 0], [2, 0.5, 0, 0]]
    recs["dir"] = [[0, 0, 1, 0], [0.6, 0.8, 0, 0], [0, -1, 0, 0]]
    recs["tri"] = [9, 0, 2]
    recs["t"] = [12.25, 0, 3.5]
    recs["face"] = [1, 0, 2]
    recs["nleaves"] = [3, 1, 1]
    recs["leaf_first"] = [0, 3, 4]
    ids = np.array([1, 2, 1, 3, 2], np.uint32)
    # stored out of (row, col) order: the CSV sorts
    rr = R.RayRecords(recs, ids, pixel=[[1, 0], [0, 1], [0, 0]])
    assert rr.leaves(0).tolist() == [1, 2, 1]
    assert rr.check_tris(0, _Tree()).tolist() == [2, 5, 7, 9]
    assert rr.counters["leaves"].tolist() == [3, 1, 1]
    f = io.StringIO()
    rr.write_csv(f, _Tree())
    assert f.getvalue() == ("Pixel_x;Pixel_y;ray_p;ray_v;tri_hit;hit_t;check_tris\n"
                            "0;0;2,0.5,0;0,-1,0;2;3.5;2,7,9\n"
                            "0;1;0.1,-0,0.0000000001;0.6,0.8,0;0;0;\n"
                            "1;0;2,0,0;0,0,1;9;12.25;2,5,7,9\n")
