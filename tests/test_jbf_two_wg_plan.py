"""The route decision of rf_jbf_u8's grey tiles (two workgroups per CU, jbf_tile64x2_kernel) as the
device-free plan query reports it, against figures derived by hand:

  LDS of a workgroup           81,920 B (half of a CU's 160 KiB), tile and LUT and nothing else
  LUT, 32 replicas             nz * 128 B at the end of the allocation
      sigma_color 20, 3-channel joint (or a 1-channel joint counted as three): float32 exp(-d * d / 800) is
      1e-45 at d = 288 and exactly 0 from d = 289 on: nz = 289 entries in front of the zero tail -> 36,992 B
      sigma_color 20, 1-channel joint counted once: d <= 255, the table never reaches zero, nz = 256 -> 32,768 B
  a tile row at pitch 144      576 B
  rows in front of the LUT     (81,920 - 36,992) // 576 = 78 exactly   (64 output rows + 14 rows of halo)
                               (81,920 - 32,768) // 576 = 85
  radii of pitch 144           r4 = radius rounded up to 4 <= 36, i.e. radius <= 36

and the size rule of the tile-flag buffer: one byte per tile of the launch, rounded up to a power of two,
4 KiB at least; none where src and joint have one channel each (nothing to vote on: one launch).
"""
import pytest

SIGMA_COLOR = 20.0


def _plan(radius, n=1, h=1080, w=1920, jcn=3, scn=3, flags=0, sigma_color=SIGMA_COLOR):
    from reflectance_filtering_amd import _ffi
    return _ffi.jbf_two_wg_plan(n, h, w, jcn, scn, 2 * radius + 1, sigma_color, max(1.0, radius / 1.5), flags)


def test_route_and_rows_by_radius(built):
    tiles = 30 * 17
    for radius in range(1, 53):
        for scn in (3, 1):
            got = _plan(radius, scn=scn)
            if radius <= 36:
                assert got == (78, tiles, 4096), (radius, scn, got)     # (a 3-channel joint: votes either way)
            else:
                assert got is None, (radius, scn, got)


def test_rows_with_a_single_channel_joint(built):
    from reflectance_filtering_amd import _ffi
    assert _plan(33, jcn=1, scn=1) == (85, 30 * 17, 0)
    assert _plan(33, jcn=1, scn=1, flags=_ffi.JBF_GREY_AS_BGR) == (78, 30 * 17, 0)
    assert _plan(33, jcn=1, scn=3, flags=_ffi.JBF_GREY_AS_BGR) == (78, 30 * 17, 4096)


def test_the_metric_launch(built):
    """256 x 1080p, c20 s22: 130,560 tiles of 64x64 (1080 = 16 x 64 + 56: the bottom rows are 64x64 tiles,
    today as before), flags in 128 KiB."""
    from reflectance_filtering_amd import _ffi
    got = _ffi.jbf_two_wg_plan(256, 1080, 1920, 3, 3, -1, 20.0, 22.0)
    assert got == (78, 130560, 131072)


def test_flag_buffer_size_rule(built):
    for n, h, w, tiles in ((1, 64, 64, 1), (1, 70, 72, 2), (64, 64, 4096, 4096), (65, 64, 4096, 4160),
                           (3, 64, 128, 6)):
        want = 4096
        while want < tiles:
            want *= 2
        got = _plan(33, n=n, h=h, w=w)
        assert got == (78, tiles, want), (n, h, w, got)


def test_strips_stay_on_the_old_kernel(built):
    """A 3-channel image of 70 x 72: the 6 rows below the first 64 are a 32x128 strip (one workgroup against
    two), so the route's launch has the two tiles of the first 64 rows; with jbf_tile64_only all four."""
    from reflectance_filtering_amd import _ffi
    assert _plan(7, h=70, w=72)[1] == 2
    with _ffi.debug_options(jbf_tile64_only=1):
        assert _plan(7, h=70, w=72)[1] == 4
    # an image that is all strip has no tile for the route
    assert _plan(7, h=10, w=300, scn=1) is None


@pytest.mark.parametrize("option", ("jbf_no_two_wg", "jbf_compiler_loop", "jbf_lookahead1", "jbf_stage_only",
                                    "jbf_tune"))
def test_switches_that_keep_the_old_path(built, option):
    from reflectance_filtering_amd import _ffi
    assert _plan(33) is not None
    with _ffi.debug_options(**{option: 7 if option == "jbf_tune" else 1}):
        assert _plan(33) is None
    assert _plan(33, flags=_ffi.JBF_FORCE_GENERIC) is None
    assert _plan(33) is not None


def test_a_wide_colour_table_is_off_the_route(built):
    """sigma_color 60: the table is 3 * 255 entries long, 32 replicas of it do not fit beside a tile - the
    tile kernel runs it at fewer replicas, and the route asks for 32."""
    assert _plan(33, sigma_color=60.0) is None


def test_refusals(built):
    from reflectance_filtering_amd import _ffi
    with pytest.raises(ValueError):
        _ffi.jbf_two_wg_plan(1, 0, 64, 3, 3, -1, 20.0, 22.0)
    with pytest.raises(ValueError):
        _ffi.jbf_two_wg_plan(1, 64, 64, 2, 3, -1, 20.0, 22.0)
    with pytest.raises(ValueError):
        _ffi.jbf_two_wg_plan(0, 64, 64, 3, 3, -1, 20.0, 22.0)
