"""fp64 restatement of the ray formula of csrc/mcnerf_rays.h (written from its comments; every ray kernel of csrc/rays.hip calls it)
for a batch that spans cameras, differentiable by autograd:

    u = pix % W + 0.5, v = pix // W + 0.5                      pixel centres, pix = v * W + u
    cam = Kinv [u, v, 1]^T                                      lift through the inverse intrinsics
    q_c = sum_j cam_j R[j][c]                                   R^T cam (pose = world->cam [R|t])
    d = q / |q|,   o_c = -sum_j R[j][c] t_j                     unit direction, origin -R^T t

Segment k of the batch is rays [seg_start[k], seg_start[k+1]) of camera seg_cam[k].  Not a test module."""
import torch


def rays(pose, kinv, seg_cam, seg_start, pix, W):
    """pose [C,3,4], kinv [C,3,3] (any float dtype; computed in fp64), pix [n] int64 -> rays_d, rays_o [n,3] fp64."""
    pose, kinv = pose.double(), kinv.double()
    cam_of_ray = torch.cat([torch.full((seg_start[k + 1] - seg_start[k],), int(c), dtype=torch.int64) for k, c in enumerate(seg_cam)])
    cam_of_ray = cam_of_ray.to(pix.device)
    P, K = pose[cam_of_ray], kinv[cam_of_ray]                   # [n,3,4], [n,3,3]
    p = torch.stack([(pix % W).double() + 0.5, torch.div(pix, W, rounding_mode="floor").double() + 0.5, torch.ones_like(pix).double()], -1)
    cam = (K @ p.unsqueeze(-1)).squeeze(-1)
    R, t = P[:, :, :3], P[:, :, 3]
    q = (R.transpose(1, 2) @ cam.unsqueeze(-1)).squeeze(-1)
    d = q / q.norm(dim=-1, keepdim=True)
    o = -(R.transpose(1, 2) @ t.unsqueeze(-1)).squeeze(-1)
    return d, o


def backward(pose, kinv, seg_cam, seg_start, pix, W, g_d, g_o):
    """d_pose [C,3,4], d_kinv [C,3,3] in fp64 for the upstream gradients g_d, g_o [n,3]."""
    pose = pose.detach().double().clone().requires_grad_(True)
    kinv = kinv.detach().double().clone().requires_grad_(True)
    d, o = rays(pose, kinv, seg_cam, seg_start, pix, W)
    ((d * g_d.double()).sum() + (o * g_o.double()).sum()).backward()
    return pose.grad, kinv.grad


def gt_from_u8(images_u8, cam, pix):
    """images_u8 [C, H*W, 3|4] uint8 -> [n,3] fp32: /255 first, then the blend on white for 4 channels (the formula of
    gather_gt_kernel, in the same fp32 order; on HOST tensors, where torch divides -- on the device it multiplies by 1 / 255)."""
    f = images_u8[cam][pix].float() / 255.0
    return f[:, :3] * f[:, 3:] + (1.0 - f[:, 3:]) if f.shape[-1] == 4 else f
