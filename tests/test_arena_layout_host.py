"""Host tier, no GPU: the layout of a fold batch's arenas and of the optional step terms' side blocks (runtime.arena_layout over
FoldArena.model_regions / FoldArena.side_regions, which allocate nothing).  The expected offsets, sizes and strides below were taken
from FoldArena as it stood BEFORE the side blocks became one table (four hand-written blocks, each with its own offsets), for
C = 3, K = 2, T = 64, a training batch of 8: nothing on, everything on, and dro + supcon only.  A term must not move another
term's block, and no term may move the model arenas."""
import torch

from multimodalsignal_amd.runtime import FoldArena, arena_layout

CC, K, T, B = 3, 2, 64, 8
MODEL = {"params": (0, 494032), "grads": (494080, 494032), "exp_avg": (988160, 494032), "exp_avg_sq": (1482240, 494032),
         "bn_state": (1976320, 384), "bn_count": (1976832, 16), "acc": (1977088, 16), "x": (1977344, 6144), "y": (1983488, 64),
         "ws": (1983744, 20074240), "cw": (22057984, 8)}
MODEL_ALL = dict(MODEL, gc=(22058240, 31224), avg_params=(22089472, 494032), avg_bn_state=(22583552, 384), avg_bn_count=(22584064, 16),
                 sam=(22584320, 494768))
SIDE = {"adversary": ({"params": (0, 34064), "exp_avg": (34304, 34064), "exp_avg_sq": (68608, 34064), "stats": (102912, 24),
                       "dom": (103168, 4000)}, 107264),
        "distill": ({"stats": (0, 24), "q": (256, 6216)}, 6656),
        "dro": ({"q": (0, 256), "stats": (256, 1552), "grp": (2048, 4000)}, 6144),
        "supcon": ({"stats": (0, 32), "grp": (256, 4936), "scratch": (5376, 4352)}, 9728)}
DTYPES = {"adversary": dict(params=torch.float32, exp_avg=torch.float32, exp_avg_sq=torch.float32, stats=torch.float64, dom=torch.int32),
          "distill": dict(stats=torch.float64, q=torch.float32), "dro": dict(q=torch.float32, stats=torch.float64, grp=torch.int32),
          "supcon": dict(stats=torch.float64, grp=torch.int32, scratch=torch.uint8)}
ALL = dict(adversary=(4, 1000), distill=777, dro=(5, 1000), supcon=1234)


def _side(**terms):
    side = FoldArena.side_regions(K, B, **terms)
    return {t: arena_layout(regs) for t, regs in side.items()}, {t: {name: dt for name, _, dt in regs} for t, regs in side.items()}


def test_model_arenas_have_the_layout_they_had():
    assert arena_layout(FoldArena.model_regions(CC, K, T, B)) == (MODEL, 22058240)
    assert arena_layout(FoldArena.model_regions(CC, K, T, B, grad_clip=True, averaging=True, sam=True)) == (MODEL_ALL, 23079168)
    off, stride = arena_layout(FoldArena.model_regions(CC, K, T, B, grad_clip=True, averaging=True, sam=True))
    assert list(off) == list(MODEL_ALL) and stride % 256 == 0 and all(o % 256 == 0 for o, _ in off.values())      # order and alignment


def test_side_blocks_have_the_layout_they_had():
    assert _side() == ({}, {})
    layout, dtypes = _side(**ALL)
    assert layout == {t: SIDE[t] for t in ("adversary", "distill", "dro", "supcon")} and dtypes == DTYPES
    assert [list(layout[t][0]) for t in layout] == [list(SIDE[t][0]) for t in layout]                                # region order
    layout, dtypes = _side(dro=ALL["dro"], supcon=ALL["supcon"])
    assert layout == {"dro": SIDE["dro"], "supcon": SIDE["supcon"]} and dtypes == {t: DTYPES[t] for t in ("dro", "supcon")}
    assert set(FoldArena.SIDE_ARGS) == set(SIDE)
