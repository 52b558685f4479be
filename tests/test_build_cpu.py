"""CPU: post-build checks of the shipped library's code objects (no GPU needed).

The AGPR-resident Gram kernels (gram_narrow / gram_plan / gram_cyclic) keep loop-carried accumulators in named AGPRs that
their inline-asm blocks only list as clobbers; tools/check_agpr_kernels.py verifies on the built libdlsa_hip.so that the
compiler left those registers alone: no scratch, the planned AGPR counts, VGPR + AGPR within two waves per SIMD, and no
v_accvgpr moves inside any loop of the kernels' control-flow graphs."""
import os
import shutil
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_agpr_resident_kernels_are_untouched_by_the_compiler():
    import check_agpr_kernels as chk
    lib = os.path.join(ROOT, "dlsa_amd", "libdlsa_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libdlsa_hip.so has not been built (run `make`)")
    if not (os.path.exists(chk.tool("llvm-objdump")) or shutil.which("llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    n, problems = chk.check(lib)
    # 2 weights x (narrow: NT 3..6 x G 0..3 + NT 7) + cyclic 2 x 4 + the plan kernels (weighted only)
    assert n >= 140, "only %d AGPR-resident kernels found in the library" % n
    assert not problems, "\n".join("%s: %s" % (k, "; ".join(e)) for k, e in problems)


def test_loop_detection_flags_a_move_inside_a_loop():
    """The checker's CFG / strongly-connected-component pass on a hand-made instruction list."""
    import check_agpr_kernels as chk
    ins = [(0, "s_mov_b32", None), (4, "v_accvgpr_write_b32", None),            # prologue
           (8, "v_mfma_f64_16x16x4_f64", None), (16, "v_accvgpr_read_b32", None), (20, "s_cbranch_scc1", 8),   # loop 8..20
           (24, "v_accvgpr_read_b32", None), (28, "s_endpgm", None)]            # epilogue
    inloop, nblocks = chk._cyclic_blocks(ins)
    assert nblocks == 1 and inloop == {8, 16, 20}
    # a forward jump over a block and a backward JUMP that is not a cycle (layout artefact) are not loops
    ins2 = [(0, "s_branch", 12), (4, "v_accvgpr_read_b32", None), (8, "s_endpgm", None), (12, "s_nop", None), (16, "s_branch", 4)]
    inloop2, nblocks2 = chk._cyclic_blocks(ins2)
    assert nblocks2 == 0 and not inloop2


def test_grid_barriers_drain_every_wave_before_the_arrival():
    """The grid barriers of lars_c / lars_q / lars.hip (both builds) / irls_small: on the shipped code objects, no global store
    reaches the workgroup barrier in front of an arrival (s_barrier, buffer_wbl2, global_atomic_add) without an s_waitcnt vmcnt(0)
    -- thread 0's release orders only its own wave's stores."""
    import check_grid_barriers as chk
    lib = os.path.join(ROOT, "dlsa_amd", "libdlsa_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libdlsa_hip.so has not been built (run `make`)")
    if not (os.path.exists(chk.tool("llvm-objdump")) or shutil.which("llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    kernels, problems = chk.check(lib)
    # lars_c 1 + lars_q 2 (the LDS-resident builds run on one workgroup) + lars.hip's grid kernel 2 + irls_small 4
    assert len(kernels) >= 9, sorted(kernels)
    assert not problems, "\n".join("%s: %s" % p for p in problems)


def test_grid_barrier_check_flags_a_store_that_is_not_waited_for():
    """The checker on hand-made instruction lists: __syncthreads() alone (lgkmcnt) in front of thread 0's release is flagged, also
    when the wait comes before the last store; a vmcnt(0) in every wave after the stores passes."""
    import check_grid_barriers as chk

    def arrival(pre):
        ins = [(0, "global_store_dwordx2", "v[0:1], v[2:3], off", None)] + pre + [
            (20, "s_waitcnt", "lgkmcnt(0)", None), (24, "s_barrier", "", None), (28, "s_cbranch_execz", "", 48),
            (32, "buffer_wbl2", "sc1", None), (40, "s_waitcnt", "vmcnt(0)", None), (44, "global_atomic_add", "v1, v2, s[0:1]", None),
            (48, "s_endpgm", "", None)]
        return chk.arrivals(ins)

    bad = arrival([])
    assert len(bad) == 1 and bad[0][2] == 0
    assert arrival([(8, "buffer_wbl2", "sc1", None), (16, "s_waitcnt", "vmcnt(0) lgkmcnt(0)", None)])[0][2] is None
    # a loop whose head waits, with a store after the wait: 8 store -> 12 -> 16 -> 20 barrier
    loop = [(0, "s_waitcnt", "vmcnt(0)", None), (4, "s_barrier", "", None), (8, "global_store_dword", "v0, v1, off", None),
            (12, "s_cbranch_scc1", "", 0), (16, "s_waitcnt", "lgkmcnt(0)", None), (20, "s_barrier", "", None),
            (24, "buffer_wbl2", "sc1", None), (28, "global_atomic_add", "v1, v2, s[0:1]", None), (32, "s_endpgm", "", None)]
    arr = chk.arrivals(loop)
    assert len(arr) == 1 and arr[0][2] == 2
