"""Shared by the model-error tests: numpy / torch-on-CPU restatements, written from the cited lines, of what
vv_err_accum, vv_err_finalize, vv_r_fill, problem.init_q_matrix and problem.static_r_table compute, and the bounds the
tests hold the order-dependent sums to.

  calculate_q          model/model.py:469-490   error_var (fp64) += ((output - target)**2 in fp32), / total_step
  init_q_matrix        da_4dvar.py:528-550      per window slot the grid mean of q%d.npy, broadcast
  get_static_info R    da_4dvar.py:630-634      R[0] = obs_var, R[i+1] = obs_var + q[i] assigned into an fp32 tensor
"""
import os

import numpy as np
import torch

U = 2.0 ** -53  # the unit roundoff of fp64


def sum_bound(n_terms: int) -> float:
    """Two fp64 sums of the same n terms of one sign, in any two orders, differ by at most 2 n 2^-53 relative: each
    is within (n - 1) u (1 + O(n u)) of the exact sum (Higham, Accuracy and Stability, eq. 4.4). For terms of mixed
    sign the same factor multiplies the sum of the magnitudes."""
    return 2.0 * n_terms * U


def accumulate_ref(error_var: np.ndarray, outputs, targets) -> np.ndarray:
    """error_var += ((output - target)**2).numpy() sample by sample (:485-486): fp32 difference, fp32 square, fp64
    add. outputs, targets: sequences of (C, H, W) fp32 arrays; error_var (C, H, W) fp64, updated in place."""
    assert error_var.dtype == np.float64
    for o, t in zip(outputs, targets):
        o = torch.from_numpy(np.ascontiguousarray(o, np.float32))
        t = torch.from_numpy(np.ascontiguousarray(t, np.float32))
        sq = (o - t) ** 2
        assert sq.dtype == torch.float32
        error_var += sq.numpy()
    return error_var


def diff_sums_ref(outputs, targets):
    """(sum of (double)(output - target) per channel, sum of its magnitudes per channel) over all samples, fp64."""
    s = a = 0.0
    for o, t in zip(outputs, targets):
        d = (np.asarray(o, np.float32) - np.asarray(t, np.float32)).astype(np.float64)
        s = s + d.sum((1, 2))
        a = a + np.abs(d).sum((1, 2))
    return s, a


def calculate_q_ref(outputs, targets) -> np.ndarray:
    """calculate_q (:469-490) given the model outputs: one sample per step, total_step = the number of samples."""
    outputs = list(outputs)
    ev = accumulate_ref(np.zeros(np.shape(outputs[0]), np.float64), outputs, targets)
    return ev / len(outputs)


def init_q_matrix_ref(coeff_dir: str, q_type: int, da_win: int, nchannel: int, nlat: int, nlon: int):
    """init_q_matrix (:528-550) on CPU tensors; the q_type 1 branch resizes to (nlat, nlon) where the reference
    writes its own grid (721, 1440). Returns the (da_win - 1, nchannel, nlat, nlon) tensor, [] for da_win 1."""
    import torch.nn.functional as F

    if da_win == 1:
        return []
    if q_type == 0:
        q = []
        for i in range(1, da_win):
            q0 = torch.from_numpy(np.load(os.path.join(coeff_dir, "q%d.npy" % i)))
            q.append(torch.broadcast_to(torch.mean(q0, (1, 2), True), (nchannel, nlat, nlon)))
        q = torch.stack(q, 0)
    elif q_type == -1:
        q = torch.zeros(da_win - 1, nchannel, nlat, nlon)
    elif q_type == 1:
        t = torch.from_numpy(np.load(os.path.join(coeff_dir, "new_q.npy"))).unsqueeze(2).unsqueeze(2)[:da_win - 1]
        q = F.interpolate(torch.broadcast_to(t, (da_win - 1, nchannel, nlat, nlon)), size=(nlat, nlon))
    else:
        raise NotImplementedError("not implemented q type")
    return q


def static_r_ref(obs_var: torch.Tensor, q_matrix, da_win: int, nlat: int, nlon: int) -> torch.Tensor:
    """get_static_info's R (:630-634): obs_var (C, 1, 1) fp32 as data_reader holds it, q_matrix[i] (C, nlat, nlon) of
    any float dtype; the sum is formed in the promoted dtype and rounded by the assignment into the fp32 R."""
    R = torch.zeros(da_win, obs_var.shape[0], nlat, nlon)
    R[0] = obs_var
    for i in range(da_win - 1):
        R[i + 1] = obs_var + q_matrix[i]
    return R


def moments_ref(error_var: np.ndarray, diff_sum: np.ndarray, n_samples: int):
    """Per channel mean and variance of the error over the N = n H W differences: sum d / N, sum d^2 / N - mean^2."""
    N = float(n_samples) * error_var.shape[1] * error_var.shape[2]
    mean = diff_sum / N
    return mean, error_var.sum((1, 2)) / N - mean * mean
