"""The d_work sizes of the seekable rewrite calls (update, append, splice, rechunk, compose) and of the chunked encode, pinned: each
*_workspace function is asked for the same argument tuples that were put to the build of the commit before the calls' slot table, piece
table and re-encode step got one owner (csrc/frame_rewrite_device.h), and must answer what that build answered.  The carve may be shared;
what it adds up to may not move.  Host arithmetic only: no GPU.

The tuples of each function: no stream (and, for compose, no output); one of everything; max_slots = 0; stage_cap = 0 (or, for the two calls
without one, max_tails = 0 / max_chunks = 0); chunk_bytes 1, 4096 and 65536 on one middling batch; a chunk size the call refuses (0 or
65537); and one large batch (163 840 streams, 2^20 slots, 4 GiB of staging)."""
import pytest

BIG_NS, BIG_M, BIG_SC = 163840, 1 << 20, 1 << 32

# function -> (the loader in snappier_amd._native, [(arguments, bytes)])
PINS = {
    # nstreams, nreq, max_slots, stage_cap
    "snp_frame_write_indexed_workspace": ("frame_update_lib", [
        ((0, 5, 10, 1000), 0),
        ((5, 0, 10, 1000), 0),
        ((1, 1, 1, 1), 12032),
        ((3, 7, 0, 1000), 8704),
        ((3, 7, 10, 0), 13312),
        ((300, 1025, 2000, 70000), 809216),
        ((1025, 3, 255, 1048576), 2434816),
        ((BIG_NS, BIG_NS, BIG_M, BIG_SC), 9621132800),
    ]),
    # nstreams, max_tails, max_slots, chunk_bytes
    "snp_frame_append_indexed_workspace": ("frame_append_lib", [
        ((0, 5, 10, 4096), 0),
        ((1, 1, 1, 4096), 24576),
        ((3, 3, 0, 4096), 35840),
        ((3, 0, 10, 4096), 55040),
        ((300, 300, 2000, 1), 298240),
        ((300, 300, 2000, 4096), 12493056),
        ((300, 300, 2000, 65536), 195789056),
        ((3, 3, 10, 0), 0),
        ((3, 3, 10, 65537), 0),
        ((BIG_NS, BIG_NS, BIG_M, 65536), 103578904064),
    ]),
    # nstreams, max_slots, stage_cap, chunk_bytes
    "snp_frame_splice_indexed_workspace": ("frame_splice_lib", [
        ((0, 10, 1000, 4096), 0),
        ((1, 1, 1, 4096), 16128),
        ((3, 0, 1000, 4096), 10240),
        ((3, 10, 0, 4096), 59392),
        ((300, 2000, 70000, 1), 367616),
        ((300, 2000, 70000, 4096), 9903616),
        ((300, 2000, 70000, 65536), 153263616),
        ((3, 10, 1000, 0), 0),
        ((3, 10, 1000, 65537), 0),
        ((BIG_NS, BIG_M, BIG_SC, 65536), 84610721536),
    ]),
    # nstreams, max_slots, stage_cap, chunk_bytes, max_entries
    "snp_frame_rechunk_indexed_workspace": ("frame_rechunk_lib", [
        ((0, 10, 1000, 4096, 50), 0),
        ((1, 1, 1, 4096, 1), 15872),
        ((3, 0, 1000, 4096, 50), 8192),
        ((3, 10, 0, 4096, 50), 59648),
        ((3, 10, 1000, 4096, 0), 59648),
        ((300, 2000, 70000, 1, 5000), 529920),
        ((300, 2000, 70000, 4096, 5000), 10065920),
        ((300, 2000, 70000, 65536, 5000), 153425920),
        ((3, 10, 1000, 0, 50), 0),
        ((BIG_NS, BIG_M, BIG_SC, 65536, 1 << 21), 84684458496),
    ]),
    # nstreams, nout, nsegs, max_slots, stage_cap, chunk_bytes, max_entries  (nothing is kept per source stream: without one the size stays)
    "snp_frame_compose_indexed_workspace": ("frame_compose_lib", [
        ((0, 3, 5, 10, 1000, 4096, 50), 65280),
        ((3, 0, 5, 10, 1000, 4096, 50), 0),
        ((1, 1, 1, 1, 1, 4096, 1), 20480),
        ((3, 3, 0, 10, 1000, 4096, 50), 61440),
        ((3, 3, 5, 0, 1000, 4096, 50), 13056),
        ((3, 3, 5, 10, 0, 4096, 50), 64256),
        ((300, 200, 1025, 2000, 70000, 1, 5000), 665600),
        ((300, 200, 1025, 2000, 70000, 4096, 5000), 10201600),
        ((300, 200, 1025, 2000, 70000, 65536, 5000), 153561600),
        ((BIG_NS, BIG_NS, 300001, BIG_M, BIG_SC, 65536, 1 << 21), 84720032256),
    ]),
    # nbuffers, max_chunks, chunk_bytes
    "snp_frame_encode_chunked_workspace": ("frame_chunked_lib", [
        ((0, 10, 4096), 0),
        ((1, 1, 4096), 7680),
        ((3, 0, 4096), 1024),
        ((300, 2000, 1), 220416),
        ((300, 2000, 4096), 9756416),
        ((300, 2000, 65536), 153116416),
        ((3, 10, 0), 0),
        ((BIG_NS, BIG_M, 65536), 80276105472),
    ]),
}


@pytest.mark.parametrize("name", list(PINS))
def test_workspace_sizes_are_those_of_the_commit_before_the_shared_carve(name):
    from snappier_amd import _native as N
    loader, cases = PINS[name]
    assert len(cases) >= 6
    ws = getattr(getattr(N, loader)(), name)
    assert [(args, ws(*args)) for args, _ in cases] == cases
