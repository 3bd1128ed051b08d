"""A cell segmentation net of the flow-following kind (Stringer et al. 2021, "Cellpose: a generalist algorithm for cellular
segmentation"): the U-Net of irgen/unet.py with three output planes per image, as planer IR with seeded weights.

    planes        0: dy, 1: dx, the flow field towards the cell's centre; 2: the cell probability (a logit: foreground above 0)

`net.flow_output(planes=PLANES)` hands back the instance masks: every foreground pixel follows the flow, and the pixels that
meet at one sink are one cell (util.FlowSpec).  Seeded weights give flows without structure: the masks are small and many.
"""
from . import unet

PLANES = (0, 1, 2)                                        # dy, dx, prob
CLASSES = 3


def build(seed=0, in_ch=3, up="k2"):
    return unet.build(seed=seed, in_ch=in_ch, classes=CLASSES, up=up)


def make_input(n, seed=1, size=224, in_ch=3):
    return unet.make_input(n, seed=seed, size=size, in_ch=in_ch)
