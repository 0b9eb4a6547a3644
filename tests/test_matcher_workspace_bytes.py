"""The workspace sizes of the matcher MLP's two backward entry points are part of what callers allocate by: they are pinned here.  Both carve one shared operand
block (csrc/s2d_bwd_host.h) and the coarse matcher adds its own buffers behind it; every piece is aligned to 256 bytes, so the totals depend on the set of
pieces alone.  The library loads without a device."""
from nerf_loc_amd import _lib

# printed from a build of the commit before the two carves were merged into one (not from the code under test)
S2D_BACKWARD_TRAIN_BYTES = {(1, 1, 32): 17043968, (5, 37, 32): 17441280, (64, 300, 128): 66425856, (2048, 4096, 256): 269500416}   # (N, M, C)
FINE_MATCH_BACKWARD_BYTES = {(0, 32): 17121792, (0, 256): 33942784, (1, 32): 17121792, (1, 256): 33942784, (7, 32): 17614080, (7, 256): 34698496,
                             (4096, 32): 353173504, (4096, 256): 549781504}   # (M, C)


def test_matcher_backward_workspace_bytes_are_pinned():
    lib = _lib.load()
    assert {k: lib.nl_s2d_backward_train_workspace_bytes(*k) for k in S2D_BACKWARD_TRAIN_BYTES} == S2D_BACKWARD_TRAIN_BYTES
    assert {k: lib.nl_fine_match_backward_workspace_bytes(*k) for k in FINE_MATCH_BACKWARD_BYTES} == FINE_MATCH_BACKWARD_BYTES
