"""The key index of an AMPC table restated for the tests (stract_amd/csrc/hb_table.hip.h, ensure_room / rebuild_index of hb_ampc.hip): the
home slot of a key and the size of the index.  Plain Python; tests/test_ampc_approx.py and tests/ampc_model.py choose their keys with it."""
M64 = (1 << 64) - 1
FIRST_SLOTS = 1024  # the smallest index


def slot_hash(key):
    """slot_hash() of stract_amd/csrc/hb_table.hip.h restated: the home slot of a key is slot_hash(key) & (slots - 1)"""
    x = (key & M64) ^ (((key >> 64) * 0x9E3779B97F4A7C15) & M64)
    for _ in range(2):
        x ^= x >> 32
        x = (x * 0xD6E8FEB86659FD93) & M64
    return x ^ (x >> 32)


def slots_for(keys):
    """rebuild_index: 1024 slots, or the power of two at or above 2 x keys"""
    slots = FIRST_SLOTS
    while slots < 2 * keys:
        slots <<= 1
    return slots


def keys_with_home(home, slots, count, high=0, start=1):
    """the first `count` ids start, start + 1, ... (with `high` as their upper half) whose home slot in an index of `slots` is `home`"""
    out, k = [], start
    while len(out) < count:
        key = k | (high << 64)
        if slot_hash(key) & (slots - 1) == home:
            out.append(key)
        k += 1
    return out
