"""The pedigree check's kernels (csrc/vcf_pedcheck_dev.h) keep every value in registers: no scratch, read from the built gfx950
code object's metadata as tests/test_cpu_kernel_resources.py reads it for the others (no GPU needed)."""
import pytest

from test_cpu_kernel_resources import _resources

VPC_KERNELS = [
    "k_vcf_pedcheck_lean(DevArgs, VpcArgs)",
    "k_vcf_pedcheck_nuc(DevArgs, VpcArgs)",
    "void k_vcf_pedcheck_es<true>(DevArgs, VpcArgs)",
    "void k_vcf_pedcheck_es<false>(DevArgs, VpcArgs)",
]


@pytest.fixture(scope="module")
def res():
    return _resources()


def test_pedcheck_kernels_use_no_scratch(res):
    for k in VPC_KERNELS:
        assert k in res, [n for n in res if "pedcheck" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])
