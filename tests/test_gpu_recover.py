"""GPU suite: the three device entries of librf_recover_hip.so against the float32 restatement
(tests/recover_numpy.py), bit for bit: on the eight cases of the reference's own layers (tests/golden/recover.npz)
and on seeded inputs at the sizes where the boundary kernel takes another path (P = 1, 63, 64, 65; the plan's pass
size - 1, exact, + 1; workgroups x pass + 1, where one workgroup takes a second pass; a run cut from the middle of
a larger buffer at a base that is not 256-byte aligned).  loss_out is the restatement's ordered float64 sum, the
same over 0x00 / 0xA5 / 0xFF workspaces and from run to run."""
import ctypes

import numpy as np
import pytest

from tests import recover_cases as RC
from tests import recover_numpy as restate
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


class Dev(object):
    def __init__(self, env):
        self.rf, _, self.torch = env
        from reflectance_filtering_amd import _ffi_recover
        self.ffi = _ffi_recover
        self.lib = self.ffi.load_library()

    def up(self, array):
        return self.torch.from_numpy(np.ascontiguousarray(array)).cuda()

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def ok(self, rc):
        assert rc == 0, self.lib.rf_recover_last_error()

    def forward(self, x, e, pixel, norm):
        torch = self.torch
        count = len(e) if pixel is None else len(pixel)
        outs = [torch.full((count,), np.nan, dtype=torch.float32, device="cuda"),
                torch.full((count, 3), np.nan, dtype=torch.float32, device="cuda"),
                torch.full((count,), np.nan, dtype=torch.float32, device="cuda")]
        dx, de = self.up(x), self.up(e)
        dp = None if pixel is None else self.up(pixel)
        self.ok(self.lib.rf_recover_forward_f32(dx.data_ptr(), de.data_ptr(), len(e),
                                                None if dp is None else dp.data_ptr(), count, norm,
                                                outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                self.stream()))
        torch.cuda.synchronize()
        return dict(zip(("lightness", "reflectance", "shading"), (o.cpu().numpy() for o in outs)))

    def boundary(self, dx, de, npixels, norm, penalty, scale_r, scale_s, ws_byte=0xA5):
        """dx, de: device tensors whose data_ptr() is the first pixel of the run."""
        torch = self.torch
        need = self.ffi.boundary_workspace_bytes(npixels)
        ws = torch.full((need,), ws_byte, dtype=torch.uint8, device="cuda")
        means = torch.full((2,), np.nan, dtype=torch.float64, device="cuda")
        grad = torch.full((npixels + 2,), np.nan, dtype=torch.float32, device="cuda")      # a guard at either end
        self.ok(self.lib.rf_recover_boundary_backward_f32(dx.data_ptr(), de.data_ptr(), npixels, norm, penalty,
                                                          scale_r, scale_s, means.data_ptr(), grad.data_ptr() + 4,
                                                          ws.data_ptr(), need, self.stream()))
        torch.cuda.synchronize()
        grad = grad.cpu().numpy()
        assert np.isnan(grad[0]) and np.isnan(grad[-1]), "grad_e was written outside its P elements"
        return {"loss_out": means.cpu().numpy(), "grad_e": grad[1:-1].copy()}


    def scatter(self, x, e, grad_l, pixel, norm, scale, grad_e):
        """grad_e (host) after the scatter entry, behind guards."""
        torch = self.torch
        guarded = torch.full((len(e) + 2,), np.nan, dtype=torch.float32, device="cuda")
        guarded[1:-1] = self.up(grad_e)
        dx, de, dl, dp = self.up(x), self.up(e), self.up(grad_l), self.up(pixel)
        self.ok(self.lib.rf_recover_hinge_scatter_f32(dx.data_ptr(), de.data_ptr(), dl.data_ptr(), dp.data_ptr(),
                                                      len(pixel), len(e), norm, scale, guarded.data_ptr() + 4,
                                                      self.stream()))
        got = guarded.cpu().numpy()
        assert np.isnan(got[0]) and np.isnan(got[-1]), "grad_e was written outside its P elements"
        return got[1:-1].copy()


@pytest.fixture(scope="module")
def dev(env):
    return Dev(env)


def same(got, want, what):
    for name in want:
        RC._same_bits(got[name], want[name], "%s %s" % (what, name))


def test_the_eight_fixture_cases_bit_for_bit(dev):
    for c in RC.fixture_cases():
        what = "%s penalty %d" % (c["mode"], c["penalty"])
        got = dev.forward(c["x"], c["e"], None, c["norm"])
        # the reference's own tops, and the restatement's lightness
        RC._same_bits(got["reflectance"], np.ascontiguousarray(c["refl"][:, ::-1]), what + " reflectance")
        RC._same_bits(got["shading"], np.ascontiguousarray(c["shading"][:, 0]), what + " shading")
        RC._same_bits(got["lightness"], restate.recover32(c["x"], c["e"], c["norm"])["lightness"], what)
        out = dev.boundary(dev.up(c["x"]), dev.up(c["e"]), len(c["e"]), c["norm"], c["penalty"], c["scale"],
                           c["scale"])
        RC._same_bits(out["grad_e"], c["diff"], what + " grad_e against the reference's bottom[0].diff")
        same(out, RC.boundary_oracle(dev.rf, c["x"], c["e"], c["norm"], c["penalty"], c["scale"], c["scale"]), what)
        # the hinge scatter on top of it, at a list of points
        pixel = RC.pixel_list(len(c["e"]), 200, 7)
        grad_l = np.random.RandomState(8).uniform(-1, 1, 200).astype(np.float32)
        grad_e = dev.up(out["grad_e"])
        dx, de, dl, dp = dev.up(c["x"]), dev.up(c["e"]), dev.up(grad_l), dev.up(pixel)
        dev.ok(dev.lib.rf_recover_hinge_scatter_f32(dx.data_ptr(), de.data_ptr(), dl.data_ptr(), dp.data_ptr(), 200,
                                                    len(c["e"]), c["norm"], 10.0, grad_e.data_ptr(), dev.stream()))
        want = restate.hinge_scatter32(c["x"], c["e"], grad_l, pixel, c["norm"], 10.0, out["grad_e"])
        RC._same_bits(grad_e.cpu().numpy(), want, what + " scatter")
        assert (want != out["grad_e"]).sum() >= 190


def sizes(dev):
    per, most, _ = dev.ffi.boundary_plan(2 ** 31 - 1)
    return [1, 63, 64, 65, per - 1, per, per + 1, per * most + 1]


def test_seeded_sizes_bit_for_bit(dev):
    per, most, _ = dev.ffi.boundary_plan(2 ** 31 - 1)
    for i, npixels in enumerate(sizes(dev)):
        norm, penalty = i % 4, 1 + i % 2
        x, e = RC.seeded(npixels, 50 + i)
        what = "P=%d norm %d penalty %d" % (npixels, norm, penalty)
        got = dev.forward(x, e, None, norm)
        same(got, RC.forward_oracle(x, e, np.arange(npixels), norm), what)
        out = dev.boundary(dev.up(x), dev.up(e), npixels, norm, penalty, 0.1, 0.25)
        same(out, RC.boundary_oracle(dev.rf, x, e, norm, penalty, 0.1, 0.25), what)
        # the scatter at every second pixel and the last one, on top of that gradient
        pixel = np.unique(np.concatenate([np.arange(0, npixels, 2), [npixels - 1]])).astype(np.int64)[::-1].copy()
        grad_l = np.random.RandomState(60 + i).uniform(-1, 1, pixel.size).astype(np.float32)
        got_e = dev.scatter(x, e, grad_l, pixel, norm, 10.0, out["grad_e"])
        RC._same_bits(got_e, restate.hinge_scatter32(x, e, grad_l, pixel, norm, 10.0, out["grad_e"]),
                      what + " scatter")
    assert dev.ffi.boundary_plan(per * most + 1) == (per, most, most)


def test_a_nan_output_stays_nan_at_its_pixel_alone(dev):
    """np.maximum hands a NaN on where fmaxf would return EPS: a diverged network must show."""
    x, e = RC.seeded(600, 77)
    e[[5, 300, 599]] = np.nan
    for norm in range(4):
        got = dev.forward(x, e, None, norm)
        want = RC.forward_oracle(x, e, np.arange(600), norm)
        out = dev.boundary(dev.up(x), dev.up(e), 600, norm, 1 + norm % 2, 0.1, 0.25)
        ref = RC.boundary_oracle(dev.rf, x, e, norm, 1 + norm % 2, 0.1, 0.25)
        got["grad_e"], want["grad_e"] = out["grad_e"], ref["grad_e"]
        for name in want:
            bad = np.isnan(want[name])
            assert bad.reshape(600, -1).any(axis=1).nonzero()[0].tolist() == [5, 300, 599], name
            assert np.array_equal(np.isnan(got[name]), bad), name
            RC._same_bits(got[name][~bad], want[name][~bad], "norm %d %s beside the NaN pixels" % (norm, name))
        RC._same_bits(out["loss_out"], ref["loss_out"], "loss_out")
        assert np.isfinite(out["loss_out"]).all()


def test_a_run_cut_from_the_middle_of_a_larger_buffer(dev):
    x, e = RC.seeded(5000, 71)
    dx, de = dev.up(x), dev.up(e)
    first, npixels = 1237, 1500                              # byte 14,844 of x and 4,948 of e
    assert dx.data_ptr() % 256 == 0 and (12 * first) % 256 and (4 * first) % 256 and (12 * first) % 16
    out = dev.boundary(dx[first:], de[first:], npixels, 0, 1, 0.1, 0.1)
    same(out, RC.boundary_oracle(dev.rf, x[first:first + npixels], e[first:first + npixels], 0, 1, 0.1, 0.1),
         "run of 1500 from pixel 1237")


def test_loss_is_the_same_over_any_workspace_and_from_run_to_run(dev):
    per, most, _ = dev.ffi.boundary_plan(2 ** 31 - 1)
    npixels = per * most + 1 + 3 * per
    x, e = RC.seeded(npixels, 81)
    dx, de = dev.up(x), dev.up(e)
    want = RC.boundary_oracle(dev.rf, x, e, 1, 2, 0.1, 0.1)
    runs = [dev.boundary(dx, de, npixels, 1, 2, 0.1, 0.1, ws_byte=b) for b in (0x00, 0xA5, 0xFF, 0xFF)]
    for out in runs:
        same(out, want, "P=%d" % npixels)


def test_zero_scales_write_exact_zeros_and_the_losses_stay(dev):
    x, e = RC.seeded(3000, 91)
    out = dev.boundary(dev.up(x), dev.up(e), 3000, 0, 1, 0.0, 0.0)
    assert (out["grad_e"] == 0).all()
    want = RC.boundary_oracle(dev.rf, x, e, 0, 1, 0.0, 0.0)
    same(out, want, "scales 0, 0")
    assert want["loss_out"].min() > 0


def test_scatter_of_a_zero_gradient_changes_nothing_and_the_ends_are_reached(dev):
    torch = dev.torch
    npixels = 4097
    x, e = RC.seeded(npixels, 95)
    rng = np.random.RandomState(96)
    start = rng.uniform(-1, 1, npixels).astype(np.float32)
    dx, de = dev.up(x), dev.up(e)
    pixel = RC.pixel_list(npixels, 500, 97)
    dp = dev.up(pixel)
    for grad_l in (np.zeros(500, np.float32), rng.uniform(-1, 1, 500).astype(np.float32)):
        guarded = torch.full((npixels + 2,), np.nan, dtype=torch.float32, device="cuda")
        guarded[1:-1] = dev.up(start)
        dl = dev.up(grad_l)
        dev.ok(dev.lib.rf_recover_hinge_scatter_f32(dx.data_ptr(), de.data_ptr(), dl.data_ptr(), dp.data_ptr(), 500,
                                                    npixels, 3, 2.5, guarded.data_ptr() + 4, dev.stream()))
        got = guarded.cpu().numpy()
        assert np.isnan(got[0]) and np.isnan(got[-1])
        want = restate.hinge_scatter32(x, e, grad_l, pixel, 3, 2.5, start)
        RC._same_bits(got[1:-1].copy(), want, "scatter")
        if not grad_l.any():
            assert np.array_equal(want, start)
        else:
            assert want[0] != start[0] and want[-1] != start[-1]        # the first and the last pixel are listed
    # two pixels, the first and the last, through the forward entry
    ends = np.array([npixels - 1, 0], dtype=np.int64)
    same(dev.forward(x, e, ends, 2), RC.forward_oracle(x, e, ends, 2), "first and last pixel")


def test_empty_calls_write_nothing_and_an_empty_mean_is_zero(dev):
    torch = dev.torch
    means = torch.full((2,), np.nan, dtype=torch.float64, device="cuda")
    dev.ok(dev.lib.rf_recover_boundary_backward_f32(None, None, 0, 0, 1, 0.1, 0.1, means.data_ptr(), None, None, 0,
                                                    dev.stream()))
    torch.cuda.synchronize()
    assert means.cpu().numpy().tolist() == [0.0, 0.0]
