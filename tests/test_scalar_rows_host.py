"""The host's rule for the three-step fp64 block strip's 32-bit row offsets (crd_kernels.h: fused_scalar_rows_addressable; crd_fused.hip:
fused_steps_supported): the kernel addresses a plane's rows by a byte offset from the lowest row a launch can address, advanced by a row
before it is wrapped or clamped -- valid while rows x pitch stays below 2^32 bytes minus one row.  Beyond that a plan that asks for three
steps per launch steps pairs, whose addressing is 64-bit, and crd_get_launch_plan says so (crd_steps_per_launch_on is what it reports,
without a context).  No device needed."""
import crdmodel_amd as crd


def test_the_predicate_at_the_limit_and_one_row_either_side():
    for nx, real in ((8192, 8), (4096, 8), (1000, 8), (8192, 4), (489, 8)):
        pitch = nx * real
        # the largest row count whose span is below 2^32 - pitch: rows * pitch < 2^32 - pitch  <=>  (rows + 1) * pitch < 2^32
        most = (2**32 - 1) // pitch - 1
        assert (most + 1) * pitch < 2**32 <= (most + 2) * pitch
        assert crd.rows_addressable(nx, most, real)
        assert not crd.rows_addressable(nx, most + 1, real)
        assert crd.rows_addressable(nx, most - 1, real) and not crd.rows_addressable(nx, most + 2, real)
    # 8192 columns of fp64: a pitch of 2^16 bytes, so 2^32 - one row is 65535 rows exactly -- not below it; one row fewer is, one more is not
    assert 65535 * 65536 == 2**32 - 65536
    assert crd.rows_addressable(8192, 65534) and not crd.rows_addressable(8192, 65535) and not crd.rows_addressable(8192, 65536)
    # (nothing to address)
    assert not crd.rows_addressable(0, 10) and not crd.rows_addressable(10, 0)


def test_a_plane_beyond_the_limit_steps_pairs():
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 8192, 3) == 3  # the headline workload: 2^29 bytes
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 65534, 3) == 3
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 65535, 3) == 2
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 65536, 3) == 2
    assert crd.steps_per_launch_on("fhn", "f64", 16384, 32767, 3) == 2 and crd.steps_per_launch_on("fhn", "f64", 16384, 32766, 3) == 3
    # what the rule does not touch: plans of fewer steps, the fp32 three-step kernel (a resource per row), Goldbeter (pairs at the most)
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 65536, 2) == 2 and crd.steps_per_launch_on("fhn", "f64", 8192, 65536, 1) == 1
    assert crd.steps_per_launch_on("fhn", "f32", 16384, 65536, 3) == 3
    assert crd.steps_per_launch_on("goldbeter", "f64", 8192, 8192, 3) == 2
    # a slab of a multi-slab run steps pairs in fp64 whatever its size
    assert crd.steps_per_launch_on("fhn", "f64", 8192, 1024, 3, single_slab=False) == 2
