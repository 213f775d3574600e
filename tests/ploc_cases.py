"""The inputs of the PLOC rebuild tests (host model and GPU) beyond those of rebuild_cases.py: triangle soups whose size puts
both ends of the search window outside the clusters, and a run of equal triangles that ends the loop exactly at the end of a
read-back batch."""
import functools

import rebuild_cases as rc

RADIUS = 8  # rt_rebuild_desc.radius = 0
BATCH = 8  # RT_PLOC_BATCH (csrc/rt_ploc.h): iterations per read-back of the cluster count

CASES = {
    "soup_17": lambda: rc.soup(2 * RADIUS + 1),  # every window of radius 8 is clipped at one end at least
    "soup_18": lambda: rc.soup(2 * RADIUS + 2),  # ... the first size with a window clipped at neither
    "soup_100": lambda: rc.soup(100),
    # 2^BATCH equal triangles halve per iteration: one cluster is left exactly when the first batch ends; copies_257 of
    # rebuild_cases needs one iteration of a second batch
    "copies_256": lambda: rc.copies(1 << BATCH),
}


@functools.lru_cache(maxsize=None)
def flat_case(name):
    return CASES[name]() if name in CASES else rc.flat_case(name)


def deformed(name):
    """(creation, current), as rebuild_cases.deformed"""
    if name in CASES:
        f = flat_case(name)
        return f, f
    return rc.deformed(name)


# (case, radius) of the host test beyond rebuild_cases.ALL at the default radius
WINDOWS = [("soup_17", RADIUS), ("soup_18", RADIUS), ("soup_100", 1), ("soup_100", 32), ("copies_256", RADIUS)]
# (case, radius) of the device test
DEVICE = [("max_leaf", 0), ("max_leaf_plus_1", 0), ("copies", 0), ("copies_256", 0), ("copies_257", 0), ("nan_vertex", 0), ("strip", 0), ("soup_17", 0),
          ("soup_18", 0), ("soup_100", 1), ("soup_100", 8), ("soup_100", 32), ("test_scene", 0), ("semesterbild", 0), ("heightfield", 0), ("shuffle", 0)]
