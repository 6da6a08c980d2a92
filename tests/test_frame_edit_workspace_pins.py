"""The d_work size of the indexed edit call (snp_frame_edit_indexed_workspace), pinned beside those of its siblings
(test_rewrite_workspace_pins.py): the function must go on answering what it answered when the call was added.  Host arithmetic only: no GPU.

The tuples: no stream; one of everything; no edit; max_slots = 0; stage_cap = 0; chunk_bytes 1, 4096 and 65536 on one middling batch; a chunk
size the call refuses (0 and 65537); and one large batch (163 840 streams, 2^24 edits, 2^20 slots, 4 GiB of staging)."""

# nstreams, nedits, max_slots, stage_cap, chunk_bytes
PINS = [
    ((0, 7, 10, 1000, 4096), 0),
    ((1, 1, 1, 1, 4096), 24576),
    ((3, 0, 10, 1000, 4096), 59904),
    ((3, 7, 0, 1000, 4096), 18688),
    ((3, 7, 10, 0, 4096), 67840),
    ((300, 1025, 2000, 70000, 1), 715776),
    ((300, 1025, 2000, 70000, 4096), 10251776),
    ((300, 1025, 2000, 70000, 65536), 153611776),
    ((3, 7, 10, 1000, 0), 0),
    ((3, 7, 10, 1000, 65537), 0),
    ((163840, 1 << 24, 1 << 20, 1 << 32, 65536), 90666177792),
]


def test_workspace_sizes_are_those_of_the_commit_that_added_the_call():
    from snappier_amd import _native as N
    ws = N.frame_edit_lib().snp_frame_edit_indexed_workspace
    assert [(args, ws(*args)) for args, _ in PINS] == PINS
