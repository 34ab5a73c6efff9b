"""Numpy model of gptqhip_moe_align (shared by tests/test_moe_grouped_cpu.py and tests/test_gpu_moe_grouped.py): the stable counting sort of the
S = T * top_k slots by expert id into 16-row units that the expert-grouped MoE ops work on (include/gptqhip.h).

    align(ids, E) -> sorted_slots int32 [16 * max_units], unit_expert int32 [max_units], num_units, status

Experts in ascending id; an expert's slots in ascending slot index (a stable argsort), padded with -1 to a multiple of 16; an expert without
slots takes no unit; ids outside [0, E) are in no unit and give status 1; both arrays are -1 past num_units."""
import numpy as np

UNIT = 16


def max_units(S: int, E: int) -> int:
    """gptqhip_moe_grouped_units: sum_e ceil(n_e / 16) <= (S + 15 * (experts with a slot)) / 16, and never more than one unit per slot."""
    if S < 1 or E < 1:
        return 0
    return min(S, (S + 15 * min(S, E)) // 16)


def align(ids: np.ndarray, E: int):
    flat = np.asarray(ids, np.int64).reshape(-1)
    S = flat.size
    mu = max_units(S, E)
    sorted_slots = np.full(UNIT * mu, -1, np.int32)
    unit_expert = np.full(mu, -1, np.int32)
    valid = (flat >= 0) & (flat < E)
    order = np.argsort(np.where(valid, flat, E), kind="stable")      # slot indices, by expert, ascending within an expert
    u = 0
    pos = 0
    for e in range(E):
        n = int((flat == e).sum())
        if n == 0:
            continue
        nu = -(-n // UNIT)
        sorted_slots[UNIT * u:UNIT * u + n] = order[pos:pos + n]
        unit_expert[u:u + nu] = e
        u += nu
        pos += n
    return sorted_slots, unit_expert, u, int(not valid.all())


def routing_cases(E: int, top_k: int):
    """name -> ids int32 [T, top_k]: the routings at which a sort can go wrong."""
    rng = np.random.RandomState(11)
    cases = {}
    cases["random_T70"] = rng.randint(0, E, size=(70, top_k))
    cases["one_expert_S40"] = np.full((40, 1), E - 1)      # three units, the last one partial
    cases["every_expert_16"] = rng.permutation(np.repeat(np.arange(E), 16)).reshape(-1, 1)
    cases["every_expert_17"] = rng.permutation(np.repeat(np.arange(E), 17)).reshape(-1, 1)
    cases["T1"] = rng.randint(0, E, size=(1, top_k))
    bad = rng.randint(0, E, size=(33, top_k))
    bad[0, 0], bad[5, top_k - 1], bad[32, 0] = -1, E, E + 7
    cases["out_of_range"] = bad
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in cases.items()}
