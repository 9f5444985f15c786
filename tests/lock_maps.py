"""The lock maps the holed-map tests share (tests/test_lock_map.py on the CPU, tests/test_gpu_lock_map.py on the GPU) and an
independent walk of the reference's graph that says which locked layers the loss gradient has to cross.

``lock`` is a per-layer argument of conv_bn / conv in the reference (yolo/yolo3_net_pos.py:71-146); its README tells users to
edit it.  Every map below has a locked layer downstream of a trainable one."""
from typing import Dict, List, Tuple

SCORE_LAYER = {4: 79, 2: 82, 1: 85}

# name -> (mask_stride, locked layers)
MAPS: Dict[str, Tuple[int, List[int]]] = {
    "hole_5_9": (2, list(range(5, 10))),
    "frozen_heads": (2, list(range(53, 76))),
    "odd": (2, list(range(1, 83, 2))),
    "stage1_hole": (2, list(range(1, 53)) + [62, 63, 64]),
    "m1_hole": (1, list(range(1, 53)) + [83, 84]),
}
# the same holes in the m = 1/4 and m = 1 nets: the rows of tests/option_matrix.py use them (the per-map tests above run MAPS)
STRIDE_MAPS: Dict[str, Tuple[int, List[int]]] = {
    "frozen_heads_m4": (4, list(range(53, 76))),
    "stage1_hole_m4": (4, list(range(1, 53)) + [62, 63, 64]),
    "odd_m4": (4, list(range(1, SCORE_LAYER[4] + 1, 2))),
    "frozen_heads_m1": (1, list(range(53, 76))),
    "stage1_hole_m1": (1, list(range(1, 53)) + [62, 63, 64]),
    "odd_m1": (1, list(range(1, SCORE_LAYER[1] + 1, 2))),
}


def lock_of(name: str) -> Tuple[int, Dict[int, bool]]:
    """(mask_stride, full lock map) of a named map"""
    m, locked = MAPS[name] if name in MAPS else STRIDE_MAPS[name]
    return m, {i: (i in locked) for i in range(1, SCORE_LAYER[m] + 1)}


def inputs_of(mask_stride: int) -> Dict[int, List[int]]:
    """layer -> the layers whose outputs it reads (0 = the image), written down from the reference's text
    (yolo/yolo3_net_pos.py:159-461), not taken from the package's table"""
    ins: Dict[int, List[int]] = {1: [0], 2: [1]}
    i = 3
    for nblocks, down in ((1, 5), (2, 10), (8, 27), (8, 44), (4, None)):
        for _ in range(nblocks):
            ins[i] = [i - 1]
            ins[i + 1] = [i, i - 1]            # 3x3 of the block, plus the block's input as shortcut (:148-151)
            i += 2
        if down:
            ins[down] = [down - 1]
            i = down + 1
    for j in range(53, 60):
        ins[j] = [j - 1]
    ins[60] = [57]
    ins[61] = [43, 60]                         # [skip5, up2(act60)] (:290-291)
    for j in range(62, 68):
        ins[j] = [j - 1]
    ins[68] = [65]
    ins[69] = [26, 68]                         # [skip4, up2(act68)] (:325-326)
    for j in range(70, 76):
        ins[j] = [j - 1]
    ins[76] = [73]
    ins[77] = [9, 76]                          # [skip3, up2(act76)] (:386-387)
    ins[78] = [77]
    ins[79] = [78]
    if mask_stride != 4:
        ins[80] = [4, 79]                      # [skip2, up2(act79)] (:401-402)
        ins[81] = [80]
        ins[82] = [81]
    if mask_stride == 1:
        ins[83] = [1, 82]                      # [skip1, up2(act82)] (:455-456)
        ins[84] = [83]
        ins[85] = [84]
    assert sorted(ins) == list(range(1, SCORE_LAYER[mask_stride] + 1))
    return ins


def pass_through(mask_stride: int, lock: Dict[int, bool]) -> List[int]:
    """locked layers with a trainable layer somewhere upstream of one of their inputs: found by walking UP from every
    locked layer (a depth-first search per layer, no shared table with the package's forward sweep)"""
    ins = inputs_of(mask_stride)

    def trainable_at_or_above(i: int, seen: set) -> bool:
        if i == 0 or i in seen:
            return False
        seen.add(i)
        return (not lock[i]) or any(trainable_at_or_above(j, seen) for j in ins[i])

    return [i for i in sorted(ins) if lock[i] and any(trainable_at_or_above(j, set()) for j in ins[i])]
