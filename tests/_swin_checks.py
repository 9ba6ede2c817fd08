"""What the SwinUNETR GPU tests share (test infrastructure): the engine's own LeakyReLU
branch decisions for the kink-consistent oracle (oracle.swin_oracle.ACT_MASKS)."""
import torch

from _compare import lrelu_act_masks

RB_LEVEL = {"encoder1.layer": 0, "encoder2.layer": 1, "encoder3.layer": 2, "encoder4.layer": 3,
            "encoder10.layer": 5, "decoder5.conv_block": 4, "decoder4.conv_block": 3,
            "decoder3.conv_block": 2, "decoder2.conv_block": 1, "decoder1.conv_block": 0}


def engine_act_masks(m, xshape):
    B, _, D, H, W = xshape
    return lrelu_act_masks(m._plan(torch.empty(xshape, device="cuda")), RB_LEVEL, B, D, H, W)
