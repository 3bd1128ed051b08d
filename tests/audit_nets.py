"""Nets and tables the plan-audit tests share (tests/test_plan_audit_q4ops.py on the host, tests/test_gpu_plan_audit.py on the GPU).
No device code is imported here."""
from planer_amd.irgen import edsr, fpn, resnet_gn, stylenet

# the tiny EDSR of tests/test_gpu_pixel_shuffle.py and the tiny ResNet-18-GN of tests/test_gpu_groupnorm.py (their TINY)
TINY_EDSR = dict(blocks=2, feats=8, size=12)
TINY_GN = dict(width=8, groups=4, classes=10, size=32)

# feature switch -> (net of small_net, the NCHW kinds its program must hold with the switch at 0, the kinds it may not hold)
SWITCHED_OFF = {
    "PLANER_HIP_INSTNORM_Q4": ("stylenet", ("instancenormalization", "pad"), ("instancenormalization_q4", "pad_q4")),
    "PLANER_HIP_LINEAR_Q4": ("fpn-resize", ("resize",), ("resize_q4", "resize_add_q4")),
    "PLANER_HIP_GROUPNORM_Q4": ("resnet_gn", ("reshape", "instancenormalization", "mul"), ("groupnorm", "groupnorm_q4")),
    "PLANER_HIP_PIXEL_SHUFFLE_Q4": ("edsr", ("reshape", "transpose"), ("pixelshuffle", "pixelshuffle_q4")),
}


def small_net(name):
    """-> (graph, blob, x) of the small net a switched-off run audits."""
    if name == "stylenet":
        return stylenet.build() + (stylenet.make_input(1, size=32),)
    if name == "fpn-resize":
        return fpn.build(via="resize") + (fpn.make_input(1, size=64),)
    if name == "resnet_gn":
        return resnet_gn.build(**TINY_GN) + (resnet_gn.make_input(2, size=TINY_GN["size"]),)
    return edsr.build(**TINY_EDSR, scale=2) + (edsr.make_input(2, size=TINY_EDSR["size"]),)
