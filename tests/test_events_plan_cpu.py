"""ec_events_sort_workspace_bytes without a GPU: the bytes the events-to-frames launch plan finds worth allocating, pinned
at every boundary of the plan (csrc/events.hip, events_plan).  The numbers are those of the size function that preceded
the plan, a hand-kept second copy of the launch's decisions; the rows marked "no launch uses it" are the ones where that
copy named bytes its own launch never touched, and are 0 by intent."""
import ctypes

import pytest

FLAGS = 65536                 # per-frame redo flags of the 10-bit kernels


def _b10(bands, max_frame_events):
    """flags + per CU one region of band-local codes: [band][16 waves][64 * ceil(events / 1024)] words"""
    return FLAGS, bands * 16 * 64 * -(-max_frame_events // 1024) * 4


# (H, W, max_frame_events) -> (fixed bytes, bytes per compute unit)
TABLE = [
    # the three dataset sensors at their max_frame_events, and without the bound
    ((180, 240, 20000), (FLAGS, 0)),                    # N-Caltech: whole frame as 10-bit counts
    ((100, 120, 12500), (FLAGS, 0)),                    # N-Cars
    ((480, 640, 70000), _b10(6, 70000)),                # N-ImageNet: 6 row bands of 10-bit counts
    ((180, 240, 0), (FLAGS, 0)),
    ((100, 120, 0), (FLAGS, 0)),
    ((480, 640, 0), (0, 0)),                            # no bound: no regions to size, no sort slots
    # the largest H at W = 240 whose whole histogram fits as 10-bit counts, and one row more
    ((253, 240, 20000), (FLAGS, 0)),
    ((254, 240, 20000), _b10(2, 20000)),
    ((253, 240, 0), (FLAGS, 0)),
    ((254, 240, 0), (0, 0)),
    # banded path, one W per gcd(W, 12): rows per band are whole groups of 12 pixels
    ((4000, 17, 5000), _b10(2, 5000)),                  # gcd 1
    ((2000, 34, 5000), _b10(2, 5000)),                  # gcd 2
    ((2000, 33, 5000), _b10(2, 5000)),                  # gcd 3
    ((300, 304, 5000), _b10(2, 5000)),                  # gcd 4
    ((1100, 66, 5000), _b10(2, 5000)),                  # gcd 6
    ((260, 240, 2000), _b10(2, 2000)),                  # gcd 12: two bands of 130 rows (tests/test_events_gpu.py)
    ((346, 260, 12500), _b10(2, 12500)),
    ((720, 1280, 200000), _b10(16, 200000)),
    # the region capacity steps at multiples of 1024 events
    ((480, 640, 1), _b10(6, 1)),
    ((480, 640, 1024), _b10(6, 1024)),
    ((480, 640, 1025), _b10(6, 1025)),
    # W = 640 holds 90 rows per 10-bit band: 1440 rows are B10_MAX_BANDS = 16 bands, 1441 are left to the 32-bit kernel's
    # sort slots (30 rows per band there), one slot of max_frame_events indices per compute unit
    ((1440, 640, 70000), _b10(16, 70000)),
    ((1441, 640, 70000), (0, 70000 * 4)),
    ((1441, 640, 1000), (0, 1000 * 4)),
    ((1920, 640, 70000), (0, 70000 * 4)),               # 64 sort bands = EV_SORT_MAX_BANDS
    ((1921, 640, 70000), (0, 0)),                       # 65 sort bands: no launch uses it (was 256 * 280000)
    ((2000, 640, 70000), (0, 0)),                       # 67 sort bands: no launch uses it (was 256 * 280000)
    # W = 4913 (gcd 1: 12-row units do not fit a 10-bit band): the LDS event cache is taken up to 8 bands of 4 rows
    ((12, 4913, 100), (FLAGS, 0)),
    ((13, 4913, 100), (0, 0)),
    ((32, 4913, 100), (0, 0)),                          # 8 bands: cached
    ((33, 4913, 100), (0, 100 * 4)),                    # 9 bands: sort slots
    # one 32-bit band (W * 8 * H == EV_BIN_BYTES) and one row more: such a sensor always fits as 10-bit counts
    ((96, 208, 30000), (FLAGS, 0)),
    ((97, 208, 30000), (FLAGS, 0)),
    ((96, 208, 0), (FLAGS, 0)),
    # rows wider than the sort mode's band budget (153840 bytes) but not than the plain one (EV_BIN_BYTES = 159744)
    ((48, 19500, 100), _b10(16, 100)),
    ((49, 19500, 100), (0, 0)),                         # not one row per sort band: no launch uses it (was 256 * 400)
    ((100, 19500, 100), (0, 0)),                        # likewise (was 256 * 400)
    ((100, 19230, 100), (0, 0)),                        # one row per sort band, 100 bands: no launch uses it (was 256 * 400)
    ((4, 19968, 100), _b10(2, 100)),                    # the widest row a launch takes
    ((4, 19969, 100), (0, 0)),                          # too wide for any launch: no launch uses it (was 256 * 400)
    # nothing to plan
    ((0, 240, 100), (0, 0)),
    ((-1, 240, 100), (0, 0)),
    ((180, 0, 100), (0, 0)),
    ((180, -5, 100), (0, 0)),
]


@pytest.fixture(scope='module')
def library():
    from eventclip_amd import _lib
    return _lib, _lib.lib()


@pytest.fixture(scope='module')
def cus(library):
    """The device's compute units where there is a device, else the 256 the library assumes without one."""
    n = ctypes.c_int(0)
    return n.value if library[1].ec_device_info(ctypes.byref(n), None, 0) == 0 and n.value > 0 else 256


@pytest.mark.parametrize('geometry,want', TABLE, ids=['%dx%d-%d' % g for g, _ in TABLE])
def test_sort_workspace_bytes_at_the_plan_s_boundaries(geometry, want, library, cus):
    _lib, lib = library
    p = _lib.EcEventsParams()
    p.H, p.W, p.max_frame_events = geometry
    assert int(lib.ec_events_sort_workspace_bytes(ctypes.byref(p))) == want[0] + cus * want[1]


def test_sort_workspace_bytes_of_no_params(library):
    assert int(library[1].ec_events_sort_workspace_bytes(None)) == 0
