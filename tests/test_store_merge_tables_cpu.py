"""
CPU-only checks of what the four merges over every task's own values (TIES, DARE, TALL / consensus, EMR) share on the
host: the numpy tables of one plan (merge._slot_tables) and the layout of the packed mask streams
(merge._mask_stream_layout).  Every expected array is written out here.

The store of these tests: tasks A, B, C merged (store tasks g = 0, 1, 2) over four parameters in two plans --

    plan 0 (P = 3, its tasks in the order C, A, B):  entry 0 "a.w" 6 rows, all three tasks
                                                     entry 1 "b.w" 0 rows, all three tasks
                                                     entry 2 "d.w" 7 rows, none of the merged tasks
    plan 1 (P = 2, its tasks in the order A, C):     entry 0 "c.w" 5 rows, lacks task B
                                                     entry 1 belongs to no parameter of the call
"""
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def mg():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd.merge


ROWS = {"a.w": 6, "b.w": 0, "c.w": 5, "d.w": 7}
NAMES = sorted(ROWS)
# (store task g, plan task q) per parameter, as _ties_jobs leaves them: the merged tasks that have it, in store order
LIVE = {"a.w": [(0, 1), (1, 2), (2, 0)], "b.w": [(0, 1), (1, 2), (2, 0)], "c.w": [(0, 0), (2, 1)], "d.w": []}
PLAN0 = {0: "a.w", 2: "d.w", 1: "b.w"}
PLAN1 = {0: "c.w"}


def _same(got, want, dtype):
    want = np.asarray(want, dtype=dtype)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def test_slot_tables_of_two_plans(mg):
    slot_task, task_map, column = mg._slot_tables(3, PLAN0, LIVE)
    assert _same(slot_task, [[1, 2, 0], [1, 2, 0], [0, 0, 0]], np.int32)
    assert _same(task_map, [[0, 1, 2], [0, 1, 2], [-1, -1, -1]], np.int32)      # "d.w": no live slot
    assert _same(column, [0, 0, 0], np.int64)                                   # no offsets asked for
    # "c.w" lacks task B: two slots, store tasks 0 and 2 in ascending order, no gap; entry 1 is nobody's
    slot_task, task_map, column = mg._slot_tables(2, PLAN1, LIVE)
    assert _same(slot_task, [[0, 1], [0, 0]], np.int32)
    assert _same(task_map, [[0, 2], [-1, -1]], np.int32)
    assert _same(column, [0, 0], np.int64)
    for t in (slot_task, task_map, column):
        assert t.flags["C_CONTIGUOUS"]


def test_a_plan_without_a_merged_task_keeps_one_slot(mg):
    slot_task, task_map, column = mg._slot_tables(2, {1: "d.w"}, LIVE, {"d.w": 11})
    assert _same(slot_task, [[0], [0]], np.int32)
    assert _same(task_map, [[-1], [-1]], np.int32)
    assert _same(column, [0, 11], np.int64)


def test_offsets_in_sorted_name_order(mg):
    # DARE's global rows and the streams' bits over the store's own parameters are the same running sum over the sorted
    # names; a parameter without rows takes no room and shares its offset with the next one
    bit_base, total = mg._mask_stream_layout("emr_merge_parameters", NAMES, ROWS, None, None)
    assert bit_base == {"a.w": 0, "b.w": 6, "c.w": 6, "d.w": 11} and total == 18
    assert list(bit_base) == NAMES
    _, _, column = mg._slot_tables(3, PLAN0, LIVE, bit_base)
    assert _same(column, [0, 6, 11], np.int64)
    _, _, column = mg._slot_tables(2, PLAN1, LIVE, bit_base)
    assert _same(column, [6, 0], np.int64)
    # a name without an offset (the TALL run without masks hands in an empty layout) gets 0
    _, _, column = mg._slot_tables(3, PLAN0, LIVE, {})
    assert _same(column, [0, 0, 0], np.int64)
    # rows past 2^31 stay exact in the int64 column
    _, _, column = mg._slot_tables(2, PLAN1, LIVE, {"c.w": (1 << 40) + 3})
    assert _same(column, [(1 << 40) + 3, 0], np.int64)


def test_reference_keys_the_store_lacks_occupy_bits(mg):
    ref = {"z.last": torch.zeros(3), "c.w": torch.zeros(5), "a.embed": torch.zeros(2, 2), "a.w": torch.zeros(2, 3),
           "d.w": torch.zeros(7), "b.w": torch.zeros(0)}
    bit_base, total = mg._mask_stream_layout("consensus_merge_parameters", NAMES, ROWS, ref, None)
    assert bit_base == {"a.embed": 0, "a.w": 4, "b.w": 10, "c.w": 10, "d.w": 15, "z.last": 22} and total == 25
    assert list(bit_base) == sorted(ref)
    # remove_keys takes a key out of the streams; the keys behind it move up
    bit_base, total = mg._mask_stream_layout("consensus_merge_parameters", NAMES, ROWS, ref, ["a.embed", "nobody"])
    assert bit_base == {"a.w": 0, "b.w": 6, "c.w": 6, "d.w": 11, "z.last": 18} and total == 21
    # without a reference the store's own parameters are the keys, remove_keys applies to them
    bit_base, total = mg._mask_stream_layout("consensus_merge_parameters", ["a.w", "c.w"], ROWS, None, None)
    assert bit_base == {"a.w": 0, "c.w": 6} and total == 11


@pytest.mark.parametrize("who", ["consensus_merge_parameters", "emr_merge_parameters"])
def test_layout_refusals(mg, who):
    ref = {n: torch.zeros(r) for n, r in ROWS.items()}
    with pytest.raises(ValueError) as e:
        mg._mask_stream_layout(who, NAMES, ROWS, ref, ["c.w"])
    assert str(e.value) == (f"{who}: parameter 'c.w' of the store has no place in the mask streams (it is not a "
                            f"key of reference_state_dict, or remove_keys names it)")
    with pytest.raises(ValueError) as e:
        mg._mask_stream_layout(who, NAMES, ROWS, {n: x for n, x in ref.items() if n != "a.w"}, None)
    assert str(e.value) == (f"{who}: parameter 'a.w' of the store has no place in the mask streams (it is not a "
                            f"key of reference_state_dict, or remove_keys names it)")
    with pytest.raises(ValueError) as e:
        mg._mask_stream_layout(who, NAMES, ROWS, None, ["d.w"])
    assert str(e.value) == (f"{who}: parameter 'd.w' of the store has no place in the mask streams (it is not a "
                            f"key of reference_state_dict, or remove_keys names it)")
    ref["c.w"] = torch.zeros(2, 3)
    with pytest.raises(ValueError) as e:
        mg._mask_stream_layout(who, NAMES, ROWS, ref, None)
    assert str(e.value) == f"{who}: reference_state_dict['c.w'] has 6 elements, the store holds 5 rows for it"
