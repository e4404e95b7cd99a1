"""Two-view relative pose: pose, triangulation angle and the PLANAR / PANORAMIC split of the verified
pairs whose two cameras carry a focal-length prior.  Specification: tests/util_pose.py.  This build's own published rule;
parity with COLMAP's `compute_relative_pose` is unpinned.

Where the work runs
  HIP     the triangulation of every inlier of every pair under every pose candidate, the choice of the candidate and the
          exact median of its triangulation angles, all pairs in one launch (csrc/pose.hip, vc_two_view_pose)
  torch   the candidates of a chunk's pairs, batched float64 on the device: a 3x3 SVD per essential matrix, an `eigh` of
          Hn'Hn per homography — plumbing, as the refit SVDs of estimate_e are
  host    the rule on the kernel's three numbers per pair (quaternion, configuration)
"""
import numpy as np
import torch

from .. import _lib
from ._common import CONFIG_PANORAMIC, CONFIG_PLANAR, CONFIG_PLANAR_OR_PANORAMIC, _pair_batch
from .essential import project_to_essential, rot_to_quat

H_ROTATION_EPS = 1e-10      # sigma_1^2 - sigma_3^2 of Hn (middle singular value 1) below this: Hn is a rotation, t = 0


def _proper(M):
    """Batched 3x3: M where det M >= 0, else -M."""
    return torch.where((torch.linalg.det(M) < 0)[:, None, None], -M, M)


def _pack(R, t):
    """R (n, 3, 3), t (n, 3) -> (n, 12): the kernel's candidate layout."""
    return torch.cat([R.reshape(-1, 9), t], dim=1)


def e_candidates(E):
    """E float64 (n, 3, 3) -> (n, 4, 12): the four decompositions in choose_pose's order (Ra, u), (Ra, -u), (Rb, u), (Rb, -u)."""
    U, _, Vt = torch.linalg.svd(E)
    U, Vt = _proper(U), _proper(Vt)
    W = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=E.dtype, device=E.device)
    u = U[:, :, 2] / torch.linalg.norm(U[:, :, 2], dim=1, keepdim=True)
    Ra, Rb = U @ W @ Vt, U @ W.T @ Vt
    return torch.stack([_pack(Ra, u), _pack(Ra, -u), _pack(Rb, u), _pack(Rb, -u)], dim=1)


def _positive(v):
    """(n, 3) -> v or -v, so that the component of largest magnitude (the first on ties) is positive."""
    big = torch.gather(v, 1, v.abs().argmax(dim=1, keepdim=True))
    return torch.where(big < 0, -v, v)


def h_candidates(Hn):
    """Hn float64 (n, 3, 3), normalised coordinates, any scale -> (n, 4, 12): the four solutions of Hn ~ R + t n' (Ma,
    Soatto, Kosecka, Sastry, Theorem 5.19) in the order (R1, t1), (R1, -t1), (R2, t2), (R2, -t2), t at unit norm.  The
    eigenvector signs are fixed (largest component of v1 and v3 positive, v2 = v3 x v1), so the order is a function of the
    matrix alone.  A rotation: (R nearest to Hn, t = 0) in slot 0 and three unused (NaN) slots."""
    n = Hn.shape[0]
    Hn = Hn / torch.linalg.svdvals(Hn)[:, 1].clamp(min=1e-300)[:, None, None]
    Hn = _proper(Hn)
    w, V = torch.linalg.eigh(Hn.transpose(1, 2) @ Hn)                   # ascending
    w1, w3 = w[:, 2], w[:, 0]
    v1, v3 = _positive(V[:, :, 2]), _positive(V[:, :, 0])
    v2 = torch.linalg.cross(v3, v1)
    rotation = ~(w1 - w3 >= H_ROTATION_EPS)                                # also where Hn is not finite
    den = torch.sqrt((w1 - w3).clamp(min=H_ROTATION_EPS))
    a, b = torch.sqrt((1.0 - w3).clamp(min=0.0)), torch.sqrt((w1 - 1.0).clamp(min=0.0))
    out = []
    for sign in (1.0, -1.0):
        u = (a[:, None] * v1 + sign * b[:, None] * v3) / den[:, None]
        nrm = torch.linalg.cross(v2, u)
        Um = torch.stack([v2, u, nrm], dim=2)
        hv, hu = (Hn @ v2[:, :, None])[:, :, 0], (Hn @ u[:, :, None])[:, :, 0]
        Wm = torch.stack([hv, hu, torch.linalg.cross(hv, hu)], dim=2)
        R = Wm @ Um.transpose(1, 2)
        t = ((Hn - R) @ nrm[:, :, None])[:, :, 0]
        nt = torch.linalg.norm(t, dim=1, keepdim=True)
        t = torch.where(nt > 0, t / nt.clamp(min=1e-300), torch.zeros_like(t))
        out += [_pack(R, t), _pack(R, -t)]
    cand = torch.stack(out, dim=1)
    if bool(rotation.any()):
        U, _, Vt = torch.linalg.svd(torch.nan_to_num(Hn))
        R = U @ Vt
        flip = torch.tensor([1.0, 1.0, -1.0], dtype=Hn.dtype, device=Hn.device)
        R = torch.where((torch.linalg.det(R) < 0)[:, None, None], U @ torch.diag_embed(flip.expand(n, 3)) @ Vt, R)
        single = torch.full_like(cand, float("nan"))
        single[:, 0] = _pack(R, torch.zeros((n, 3), dtype=Hn.dtype, device=Hn.device))
        cand = torch.where(rotation[:, None, None], single, cand)
    return cand


def two_view_pose(xn, offsets, cand, points=False):
    """xn float64 (total, 4) inliers in normalised coordinates, offsets int32 (P + 1), cand float64 (P, 4, 12), on one GPU
    -> front int32 (P, 4), best int32 (P,), tri_angle float64 (P,), midpoints float64 (total, 3) or None."""
    if not (xn.is_cuda and xn.dtype == torch.float64 and cand.dtype == torch.float64 and offsets.dtype == torch.int32):
        raise ValueError("two_view_pose needs float64 points and candidates and int32 offsets on the GPU")
    lib = _lib.load()
    P, total = int(cand.shape[0]), int(xn.shape[0])
    xn, offsets, cand = xn.contiguous(), offsets.contiguous(), cand.contiguous()
    dev = xn.device
    front = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    best = torch.zeros((P,), dtype=torch.int32, device=dev)
    tri = torch.zeros((P,), dtype=torch.float64, device=dev)
    pts = torch.empty((total, 3), dtype=torch.float64, device=dev) if points else None
    ws_bytes = int(lib.vc_two_view_pose_workspace_bytes(P, total))
    ws = torch.empty((max(ws_bytes // 8, 1),), dtype=torch.int64, device=dev)
    _lib.check(lib.vc_two_view_pose(_lib.ptr(xn), _lib.ptr(offsets), P, _lib.ptr(cand), _lib.ptr(front), _lib.ptr(best),
                                    _lib.ptr(tri), _lib.ptr(pts), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "vc_two_view_pose")
    return front, best, tri, pts


def relative_poses(entries, device, max_error):
    """The rule for a chunk's qualifying pairs.  entries: list of dict(config, kind "E" | "F" | "H", matrix (3, 3) — E in
    normalised coordinates, or the pixel F / H —, K1, K2 (3, 3), xn float64 (n, 4) the pair's inliers)
    -> list of dict(config, qvec, tvec, tri_angle, n_front)."""
    n = len(entries)
    if n == 0:
        return []
    M = torch.from_numpy(np.stack([np.asarray(e["matrix"], np.float64).reshape(3, 3) for e in entries])).to(device)
    K1 = torch.from_numpy(np.stack([np.asarray(e["K1"], np.float64) for e in entries])).to(device)
    K2 = torch.from_numpy(np.stack([np.asarray(e["K2"], np.float64) for e in entries])).to(device)
    cand = torch.full((n, 4, 12), float("nan"), dtype=torch.float64, device=device)
    for kind in ("E", "F", "H"):
        idx = torch.tensor([i for i, e in enumerate(entries) if e["kind"] == kind], dtype=torch.int64, device=device)
        if idx.numel() == 0:
            continue
        if kind == "E":
            cand[idx] = e_candidates(M[idx])
        elif kind == "F":
            cand[idx] = e_candidates(project_to_essential(K2[idx].transpose(1, 2) @ M[idx] @ K1[idx]))
        else:
            cand[idx] = h_candidates(torch.linalg.inv(K2[idx]) @ M[idx] @ K1[idx])
    xn, offsets, _, _ = _pair_batch([np.asarray(e["xn"], np.float64).reshape(-1, 4) for e in entries], None, device)
    front, best, tri, _ = two_view_pose(xn, offsets, cand)
    front, best, tri, cand = front.cpu().numpy(), best.cpu().numpy(), tri.cpu().numpy(), cand.cpu().numpy()
    if (best < 0).any():
        raise _lib.HipLibraryError("vc_two_view_pose: the workspace did not hold the keys of every pair")
    out = []
    for i, e in enumerate(entries):
        k = int(best[i])
        r = dict(config=e["config"], qvec=rot_to_quat(cand[i, k, :9].reshape(3, 3)), tvec=cand[i, k, 9:].copy(),
                 tri_angle=float(tri[i]), n_front=int(front[i, k]))
        if e["config"] == CONFIG_PLANAR_OR_PANORAMIC:
            f = min((e["K1"][0, 0] + e["K1"][1, 1]) / 2, (e["K2"][0, 0] + e["K2"][1, 1]) / 2)
            panoramic = r["n_front"] == 0 or r["tri_angle"] < np.arctan(max_error / f)
            r["config"] = CONFIG_PANORAMIC if panoramic else CONFIG_PLANAR
            if panoramic:
                r["tvec"] = np.zeros(3)
        out.append(r)
    return out
