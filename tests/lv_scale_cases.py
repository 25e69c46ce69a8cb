"""What tests/test_live_scale_gpu.py and tests/test_live_scale_cabi.py share: the constants of the launch-group loops and of the
capped grids, read from the header and the sources by regex (so a test that is meant to take more than one launch group, or to send
a grid-stride loop through a second pass, fails loudly when someone raises the group size or a cap), the call order of the 300
sessions of a 4096-slot pool, and the ragged chunk lengths with their zero-length arrangements."""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LV_HEADER = (ROOT / "include" / "msig_lv.h").read_text()
GROUP = int(re.search(r"#define MSIG_LV_GROUP (\d+)", LV_HEADER).group(1))
MAX_SESSIONS = int(re.search(r"#define MSIG_LV_MAX_SESSIONS (\d+)", LV_HEADER).group(1))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3

POOL_SLOTS, P = 4096, 300
NAMED = (0, 63, 64, 127, 128, 191, 192, 4095)          # both sides of a bitmap word's end, the first and the last slot
FAMILY = (5, 69, 133, 4037)                            # distinct ids that are equal modulo 64
BOUNDARY = (126, 127, 128, 129, 254, 255, 256, 257)    # entries of a call on both sides of a launch group's end


def cap(source, kernel):
    """The cap on gridDim.x of `kernel`'s launch in csrc/`source`: the N of `x > N ? N : x` in the launch itself or, where the grid is
    a variable, in the last `grid = ...` statement before it."""
    src = (ROOT / "multimodalsignal_amd" / "csrc" / source).read_text()
    at = src.index(kernel + "<<<")
    m = re.search(r"> (\d+) \? \1 :", src[at:src.index(">>>", at)])
    if m is not None:
        return int(m.group(1))
    return int(re.findall(r"\bgrid = [^;]*> (\d+) \? \1 :[^;]*;", src[:at])[-1])


def blocks(work):
    """The blocks of 256 threads the host code asks for before it caps them."""
    return (int(work) + 255) // 256


def slot_order(n=P, slots=POOL_SLOTS, seed=11):
    """n distinct slots of the pool in a fixed pseudo-random order that holds NAMED and FAMILY."""
    rs = np.random.RandomState(seed)
    must = list(NAMED + FAMILY)
    rest = [int(s) for s in rs.permutation(slots) if int(s) not in must][:n - len(must)]
    order = [int(s) for s in rs.permutation(must + rest)]
    assert len(set(order)) == n > GROUP and set(must) <= set(order) and order != sorted(order) and max(order) < slots
    assert max(order) >> 6 == (slots - 1) >> 6 and len({s >> 6 for s in order}) > 32          # most words of the bitmap
    return order


CYCLE = (0, 1, 5, 8, 13, 4, 2, 3)


def chunk_lengths(tick, n=P, most=13):
    """Entry j's chunk length at `tick`, before it is cut to what the session has left: ragged, zeros among them, and
    tick 1: entries GROUP - 1 and GROUP are empty; tick 2: the whole second group; tick 3: the whole first group."""
    out = [min(most, CYCLE[(3 * j + 5 * tick) % len(CYCLE)]) for j in range(n)]
    if tick == 1:
        out[GROUP - 1] = out[GROUP] = 0
        out[GROUP - 2], out[GROUP + 1] = 5, 3
    elif tick == 2:
        out[GROUP:2 * GROUP] = [0] * GROUP
    elif tick == 3:
        out[:GROUP] = [0] * GROUP
    return out
