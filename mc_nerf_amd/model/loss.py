"""Training loss (reference: model/loss.py:4-58): rgb MSE of the coarse and fine renders plus the
normalised-pixel reprojection MSE of the calibration branch.  A handful of tiny torch ops on [N,3]
and [C,5,2] tensors; it seeds the hand-written backward of RenderTrainFn with 2(rgb-gt)/(3N)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

COLOR_CALIB_MODES = ("none", "affine")
COLOR_CALIB_REG = 1e-3      # default of "color_calib_reg": a starting value, NOT tuned


def color_calib_settings(sys_param):
    """(mode, reg) of this build's own sys_param keys "color_calib" ("none", the default, or "affine") and "color_calib_reg" (a float
    >= 0; default COLOR_CALIB_REG); a ValueError names the key."""
    mode = sys_param.get("color_calib", "none")
    if not isinstance(mode, str) or mode not in COLOR_CALIB_MODES:
        raise ValueError(f"color_calib must be one of {COLOR_CALIB_MODES}, got {mode!r}")
    reg = sys_param.get("color_calib_reg", COLOR_CALIB_REG)
    if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not 0.0 <= reg < float("inf"):
        raise ValueError(f"color_calib_reg must be a finite float >= 0, got {reg!r}")
    return mode, float(reg)


def mask_weight_setting(sys_param):
    """This build's own sys_param key "mask_weight" (DESIGN.md 4h): the weight lambda >= 0 of the alpha-mask term, a finite float (an
    int counts, a bool does not); 0.0, the default, is today's path.  A ValueError names the key.  NOT tuned: there is no recommended value."""
    w = sys_param.get("mask_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w < float("inf"):
        raise ValueError(f"mask_weight must be a finite float >= 0, got {w!r}")
    return float(w)


def dist_weight_setting(sys_param):
    """This build's own sys_param key "dist_weight" (DESIGN.md 4i): the weight lambda >= 0 of the distortion term, a finite float (an
    int counts, a bool does not); 0.0, the default, is today's path.  A ValueError names the key.  NOT tuned: there is no recommended value."""
    w = sys_param.get("dist_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w < float("inf"):
        raise ValueError(f"dist_weight must be a finite float >= 0, got {w!r}")
    return float(w)


def depth_weight_setting(sys_param):
    """This build's own sys_param key "depth_weight" (DESIGN.md 4j): the weight lambda >= 0 of the depth term, a finite float (an int
    counts, a bool does not); 0.0, the default, is today's path.  A ValueError names the key.  NOT tuned: there is no recommended value."""
    w = sys_param.get("depth_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w < float("inf"):
        raise ValueError(f"depth_weight must be a finite float >= 0, got {w!r}")
    return float(w)


class MC_NeRF_Loss(nn.Module):
    def __init__(self, sys_param, tblogger=None):
        super().__init__()
        self.sys_param = sys_param
        self.tblogger = tblogger
        self.global_step = 0
        self.img_h = sys_param["data_img_h"]
        self.img_w = sys_param["data_img_w"]
        self.color_reg = color_calib_settings(sys_param)[1]
        self.mask_weight = mask_weight_setting(sys_param)
        self.dist_weight = dist_weight_setting(sys_param)
        self.depth_weight = depth_weight_setting(sys_param)

    def forward(self, loss_dict, epoch_type):
        if "depth" in loss_dict:
            # depth mode: the other keys exactly as without it (the mask and distortion terms included), plus the depth
            # term of the two expected depths over the depth range of the renderer
            rest = dict(loss_dict)
            depth = rest.pop("depth")
            return self.forward(rest, epoch_type) + self.get_depth_loss(depth, self.sys_param["near"], self.sys_param["far"])
        self.global_step += 1
        if "dist" in loss_dict:
            # distortion mode: the other keys exactly as without it (the mask term included), plus the distortion term
            rest = {k: v for k, v in loss_dict.items() if k not in ("dist", "mask")}
            loss = self._terms(rest, epoch_type)
            if "mask" in loss_dict:
                loss = loss + self.get_mask_loss(loss_dict["mask"])
            return loss + self.get_distortion_loss(loss_dict["dist"])
        if "mask" in loss_dict:
            # mask mode: the other keys exactly as without it, plus the alpha-mask term of the two front weights
            rest = {k: v for k, v in loss_dict.items() if k != "mask"}
            return self._terms(rest, epoch_type) + self.get_mask_loss(loss_dict["mask"])
        return self._terms(loss_dict, epoch_type)

    def _terms(self, loss_dict, epoch_type):
        if set(loss_dict) == {"intr", "rgb"} and loss_dict["rgb"][0].is_cuda:
            # the NeRF stages: reprojection term (rescaled to value 1 outside the camera-only stage, :20-23) + both rgb terms,
            # value and gradients in one launch (csrc/camera.hip: train_loss_kernel)
            from .render import TrainLossFn
            pd, pt_gt = loss_dict["intr"]
            rgb_c, rgb_f, gt = loss_dict["rgb"]
            return TrainLossFn.apply(pd, pt_gt.to(pd.device), rgb_c, rgb_f, gt, self.img_h, self.img_w, epoch_type != "CAM_PARAM_EPOCH")
        if set(loss_dict) == {"intr", "rgb", "color"}:
            # the NeRF stages with the per-camera colour calibration: one launch as well (csrc/color_calib.hip) on
            # device tensors, the eager formulation of the same loss on host tensors
            weights_color, cams, seg_start = loss_dict["color"]
            pd, pt_gt = loss_dict["intr"]
            if loss_dict["rgb"][0].is_cuda:
                from .render import TrainLossCalibFn
                rgb_c, rgb_f, gt = loss_dict["rgb"]
                return TrainLossCalibFn.apply(pd, pt_gt.to(pd.device), rgb_c, rgb_f, gt, weights_color, cams, seg_start,
                                              self.img_h, self.img_w, epoch_type != "CAM_PARAM_EPOCH", self.color_reg)
            l_intr = self.get_reproject_loss(loss_dict["intr"])
            l_intr = l_intr if epoch_type == "CAM_PARAM_EPOCH" else l_intr / (l_intr.detach() + 1e-8)
            return l_intr + self.get_rgb_loss_calibrated(loss_dict["rgb"], weights_color, cams, seg_start)
        total = 0.0
        if "intr" in loss_dict:
            l_intr = self.get_reproject_loss(loss_dict["intr"])
            # outside the camera-only stage the term is rescaled to value 1 (model/loss.py:20-23)
            total = total + (l_intr if epoch_type == "CAM_PARAM_EPOCH" else l_intr / (l_intr.detach() + 1e-8))
        if "extr" in loss_dict:
            total = total + self.get_reproject_loss(loss_dict["extr"])
        if "rgb" in loss_dict:
            total = total + self.get_rgb_loss(loss_dict["rgb"])
        return total

    def get_rgb_loss(self, rgbs_list):
        rgb_c, rgb_f, gt = rgbs_list
        loss = F.mse_loss(rgb_c, gt)
        if rgb_f is not None:
            loss = loss + F.mse_loss(rgb_f, gt)
        return loss

    def get_mask_loss(self, mask_list, weight=None):
        """weight * (mean (fg_c - alpha)^2 + mean (fg_f - alpha)^2) of [fg_c, fg_f | None, alpha]: the front weights [N] a mask-mode
        NeRF_Model keeps in `last_front_weight`, and the drawn pixels' alpha in [0, 1] (a float tensor [N]; MC_Model gathers it from the
        RGBA image set, a loop that drives NeRF_Model directly supplies it).  `weight` None: the model's "mask_weight".  One launch
        (render.MaskLossFn); device tensors only.  MSE, not BCE: fg can exceed 1 by roundoff, where BCE's logs are singular."""
        fg_c, fg_f, alpha = mask_list
        weight = self.mask_weight if weight is None else float(weight)
        if not 0.0 <= weight < float("inf"):
            raise ValueError(f"mask_weight must be a finite float >= 0, got {weight!r}")
        from .render import MaskLossFn
        return MaskLossFn.apply(fg_c, fg_f, alpha, weight)

    def get_distortion_loss(self, dist_list, weight=None):
        """weight * (dist_c.mean() + dist_f.mean()) of [dist_c, dist_f | None]: the per-ray distortion terms [N] a distortion-mode
        NeRF_Model keeps in `last_distortion`.  `weight` None: the model's "dist_weight".  Plain torch on the tensors' device; an empty
        ray set gives a zero that carries no gradient."""
        dist_c, dist_f = dist_list
        weight = self.dist_weight if weight is None else float(weight)
        if not 0.0 <= weight < float("inf"):
            raise ValueError(f"dist_weight must be a finite float >= 0, got {weight!r}")
        if dist_c.numel() == 0:
            return dist_c.new_zeros(())
        total = dist_c.mean()
        if dist_f is not None:
            total = total + dist_f.mean()
        return weight * total

    def get_depth_loss(self, depth_list, near, far, weight=None):
        """weight * (1 / max(n_valid, 1)) sum_valid [(s(zexp_c) - s(d))^2 + (s(zexp_f) - s(d))^2], s(z) = (z - near) / (far - near), of
        [zexp_c, zexp_f | None, d_gt]: the expected depths [N] a depth-mode NeRF_Model keeps in `last_expected_depth`, and the drawn
        pixels' targets [N] as RAY DISTANCE in world units (MC_Model gathers them from the image set's depth, a loop that drives
        NeRF_Model directly supplies them); a target is a measurement iff it is finite and > 0, a batch without one gives an exact zero.
        `weight` None: the model's "depth_weight".  Two launches (render.DepthLossFn); device tensors only."""
        zexp_c, zexp_f, d_gt = depth_list
        weight = self.depth_weight if weight is None else float(weight)
        if not 0.0 <= weight < float("inf"):
            raise ValueError(f"depth_weight must be a finite float >= 0, got {weight!r}")
        from .render import DepthLossFn
        return DepthLossFn.apply(zexp_c, zexp_f, d_gt, float(near), float(far), weight)

    def get_rgb_loss_calibrated(self, rgbs_list, weights_color, cams, seg_start, reg=None):
        """get_rgb_loss with the per-camera colour calibration weights_color [C,6], for loops that drive NeRF_Model
        directly: rays [seg_start[k], seg_start[k+1]) are camera cams[k]'s (host lists), which is modelled to observe
        (1 + w[0:3]) * rgb + w[3:6] of either render; + reg * (1/K) sum_k mean_j w[c_k, j]^2 over the non-empty segments (`reg`
        None: the model's "color_calib_reg").  Device tensors: one launch (TrainLossCalibFn); host tensors: eager torch."""
        rgb_c, rgb_f, gt = rgbs_list
        reg = self.color_reg if reg is None else float(reg)
        if reg < 0.0:
            raise ValueError(f"color_calib_reg must be >= 0, got {reg!r}")
        cams, seg_start = [int(c) for c in cams], [int(x) for x in seg_start]
        if rgb_c.is_cuda:
            from .render import TrainLossCalibFn
            return TrainLossCalibFn.apply(None, None, rgb_c, rgb_f, gt, weights_color, cams, seg_start, self.img_h, self.img_w, False, reg)
        K = len(cams)
        if len(seg_start) != K + 1 or K < 1 or seg_start[0] != 0 or seg_start[-1] != rgb_c.shape[0]:
            raise ValueError(f"seg_start must hold len(cams) + 1 entries from 0 to {rgb_c.shape[0]}, got {seg_start}")
        lens = torch.tensor([b - a for a, b in zip(seg_start, seg_start[1:])])
        cam_idx = torch.tensor(cams, dtype=torch.int64)
        w = weights_color[torch.repeat_interleave(cam_idx, lens)]                # [n,6]: the calibration of every ray's camera
        g, b = 1.0 + w[:, :3], w[:, 3:]
        loss = F.mse_loss(g * rgb_c + b, gt)
        if rgb_f is not None:
            loss = loss + F.mse_loss(g * rgb_f + b, gt)
        return loss + reg * (weights_color[cam_idx[lens > 0]] ** 2).mean(1).sum() / K

    def get_reproject_loss(self, rpro_list):
        pd, gt = rpro_list
        if pd.is_cuda:                                   # one fused kernel each way (csrc/camera.hip)
            from .render import ReprojLossFn
            return ReprojLossFn.apply(pd, gt.to(pd.device), self.img_h, self.img_w)
        lx = F.mse_loss(pd[..., 0] / self.img_w, gt[..., 0] / self.img_w)
        ly = F.mse_loss(pd[..., 1] / self.img_h, gt[..., 1] / self.img_h)
        return lx + ly
