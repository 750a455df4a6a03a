"""CPU restatement of Mapping::LandmarkTriangulation (TEST INFRASTRUCTURE ONLY).

Follows the reference's modules/mapping/mapping.cc:65-236 on the flat TemporalBuffer nrs_map_frame takes (include/nrs.h) with
the parts of modules/map/temporal_buffer.cc it uses.  The fp32 geometry and DeformableTriangulation are the twins of
oracle/triang_oracle.py, imported, not restated.  Every gate also records the quantity it compares and its threshold, so the
tests can show that no decision of a committed case hangs on the last bit (tests/test_map_oracle_cpu.py).

Snapshots are indexed 0 .. n_frames-1, oldest first; their frame ids are consecutive (Map::SetLastFrame inserts one per frame and
then increases the id, map.cc:106-118), which is what CheckRigidity's `frame_id++` walk assumes."""
import numpy as np

import triang_oracle as T
from triang_oracle import F32

TRACKED_WITH_3D, TRACKED = 0, 1
# rigid leg (mapping.cc:117-190); texts as the reference words them
R_OK, R_CLOSE, R_NOT_RIGID, R_MIDPOINT, R_PARALLAX, R_DEPTH_PREV, R_REPROJ_PREV, R_DEPTH_CUR, R_REPROJ_CUR = range(9)
RIGID_TEXT = ["ok", "Close features", "Rigidity not detected", "(TriangulateMidPoint's error: it returns none)", "Parallax error.",
              "Parallax error.", "Parallax error.", "Parallax error.", "Parallax error."]
D_SHORT, D_NAN = T.E_SHORT, 11                                    # "Short track", "NaN." (:101-102, :114)
MODE_NONE, MODE_RIGID, MODE_DEFORMABLE = 0, 1, 2


def candidates(tb):
    """GetTriangulationCandidatesIds (temporal_buffer.cc:62-74): TRACKED ids of the last snapshot, ascending (absl::btree_map order)"""
    return np.nonzero(np.asarray(tb["status"]) == TRACKED)[0].astype(np.int32)


def feature_track(tb, cand):
    """GetFeatureTrack (temporal_buffer.cc:173-183): the snapshots holding the id, oldest first"""
    return [f for f in range(tb["n_frames"]) if tb["has_kp"][f, cand]]


def check_rigidity(deform_mag, first, last, th, gates=None):
    """CheckRigidity (temporal_buffer.cc:218-227): every snapshot first .. last inclusive, float against float"""
    ok = True
    for f in range(first, last + 1):
        if gates is not None:
            gates.append(("deform_mag", float(F32(deform_mag[f])), float(F32(th))))
        if F32(deform_mag[f]) > F32(th):
            ok = False
    return ok


def neighbour_distances(tb, cand):
    """the distances GetClosestMapPointsToFeature (temporal_buffer.cc:97-141) compares with 20 and 500"""
    last = tb["n_frames"] - 1
    kp = tb["kp_xy"][last, cand]
    out = []
    for j in np.where(tb["has_kp"][last] & (tb["status"] == 0))[0]:
        if j == cand:
            continue
        dx, dy = np.float64(kp[0] - tb["kp_xy"][last, j, 0]), np.float64(kp[1] - tb["kp_xy"][last, j, 1])
        out.append(float(F32(np.sqrt(dx * dx + dy * dy))))
    return out


def rigid_triangulation(tb, cand, deform_mag, rad_per_pixel, rigidity_th=0.004, gates=None):
    """mapping.cc:117-190 for one candidate that passed the close-features test: (status, xyz float32[3])"""
    model, prm = tb["model"], tb["prm"]
    track = feature_track(tb, cand)
    cur_f, prev_f = track[0], track[-1]                            # :120-121: `current_` = front() = OLDEST, `previous_` = back() = NEWEST
    if not check_rigidity(deform_mag, cur_f, prev_f, rigidity_th, gates):
        return R_NOT_RIGID, np.zeros(3, F32)
    P = tb["poses"].astype(F32)
    kpc, kpp = tb["kp_xy"][cur_f, cand], tb["kp_xy"][prev_f, cand]
    cur_ray = T._normalized(T.unproject_f32(model, prm, *kpc))
    prev_ray = T._normalized(T.unproject_f32(model, prm, *kpp))
    Tc, Tp = P[cur_f], P[prev_f]
    X = T.triangulate_mid_point(prev_ray, cur_ray, Tp, Tc)         # :139-141
    n1 = (X - T.se3_inverse(Tc)[4:]).astype(F32)
    n2 = (X - T.se3_inverse(Tp)[4:]).astype(F32)
    par = T.rays_parallax(n1, n2)
    rpp = F32(rad_per_pixel)
    lo, hi = F32(rpp * F32(10)), F32(rpp * F32(20))
    if gates is not None:
        gates += [("parallax_lo", float(par), float(lo)), ("parallax_hi", float(par), float(hi))]
    if par < lo or par > hi:                                       # :152
        return R_PARALLAX, np.zeros(3, F32)
    for Tx, kp, e_depth, e_reproj in ((Tp, kpp, R_DEPTH_PREV, R_REPROJ_PREV), (Tc, kpc, R_DEPTH_CUR, R_REPROJ_CUR)):
        pc = T.se3_mul_point(Tx, X)
        if gates is not None:
            gates.append(("depth", float(pc[2]), 0.0))
        if pc[2] < 0:                                              # :160, :174
            return e_depth, np.zeros(3, F32)
        uv = T.project_pt(model, prm, pc)
        ex, ey = F32(kp[0]) - uv[0], F32(kp[1]) - uv[1]
        err = F32(ex * ex + ey * ey)
        if gates is not None:
            gates.append(("reproj", float(err), 5.991))
        if float(err) > 5.991:                                     # :167, :181
            return e_reproj, np.zeros(3, F32)
    return R_OK, X.astype(F32)


def landmark_triangulation(tb, deform_mag, rad_per_pixel, rigidity_th=0.004, min_track=5, index_snapshot=-1, gates=None, deformable=None):
    """mapping.cc:65-236.  deformable: optional {cand: (status, xyz)} computed earlier (the LM is slow in NumPy and does not depend on
    deform_mag / rad_per_pixel / index_snapshot).  Returns a dict: cand, rigid_status, rigid_xyz, deform_status, deform_xyz, n_rigid,
    n_deformable, mode, accepted_ids, accepted_xyz."""
    model, prm = tb["model"], tb["prm"]
    cand = candidates(tb)
    n = len(cand)
    r_st, d_st = np.zeros(n, np.int32), np.zeros(n, np.int32)
    r_xyz, d_xyz = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    n_rigid = n_def = 0
    for k, c in enumerate(cand):
        c = int(c)
        if gates is not None:
            for d in neighbour_distances(tb, c):
                gates += [("neighbour_20", d, 20.0), ("neighbour_500", d, 500.0)]
        if not T.closest_map_points(tb, c):                        # :90-95 (None = too close, [] = nothing within 500 px)
            r_st[k] = R_CLOSE
            d_st[k] = T.E_CLOSE
            continue
        if len(feature_track(tb, c)) >= min_track:                 # :97 TrackLenght
            st, xyz = deformable[c] if deformable is not None else T.deformable_triangulation(tb, c, model, prm, min_track)
            if st == T.OK and np.isnan(xyz).any():
                st = D_NAN                                         # :101-102
            d_st[k], d_xyz[k] = st, (xyz if st == T.OK else 0)
            n_def += st == T.OK
        else:
            d_st[k] = D_SHORT
        r_st[k], r_xyz[k] = rigid_triangulation(tb, c, deform_mag, rad_per_pixel, rigidity_th, gates)
        n_rigid += r_st[k] == R_OK                                 # :187-189 (a NaN position still counts)
    if n_rigid > 1.5 * n_def:                                      # :195
        mode = MODE_RIGID
    elif n_def >= 1.5 * n_rigid:                                   # :201
        mode = MODE_DEFORMABLE
    else:
        mode = MODE_NONE
    snap = tb["n_frames"] - 1 if index_snapshot < 0 else index_snapshot
    a_id, a_xyz = [], []
    for k, c in enumerate(cand):
        if mode == MODE_NONE:
            continue
        st, xyz = (r_st[k], r_xyz[k]) if mode == MODE_RIGID else (d_st[k], d_xyz[k])
        if st != 0 or np.isnan(xyz).any():                         # :196-206, :214
            continue
        if not tb["has_kp"][snap, c]:                              # :219 GetLandmarkIndexInFrame (temporal_buffer.cc:206-216)
            continue
        a_id.append(int(c))
        a_xyz.append(xyz)
    return dict(cand=cand, rigid_status=r_st, rigid_xyz=r_xyz, deform_status=d_st, deform_xyz=d_xyz, n_rigid=int(n_rigid),
                n_deformable=int(n_def), mode=mode, accepted_ids=np.array(a_id, np.int32), accepted_xyz=np.array(a_xyz, F32).reshape(-1, 3))


def deformable_leg(tb, min_track=5):
    """the deformable results of every candidate that reaches DeformableTriangulation, for landmark_triangulation(deformable=...)"""
    out = {}
    for c in candidates(tb):
        c = int(c)
        if T.closest_map_points(tb, c) and len(feature_track(tb, c)) >= min_track:
            out[c] = T.deformable_triangulation(tb, c, tb["model"], tb["prm"], min_track)
    return out


def margin_exceptions(gates, ulps=16):
    """gate quantities closer to their threshold than `ulps` fp32 ulp of the quantity (a NaN is decided by its being a NaN, not by a bit)"""
    bad = []
    for name, q, th in gates:
        if np.isnan(q):
            continue
        if abs(q - th) <= ulps * float(np.spacing(F32(abs(q)))):
            bad.append((name, q, th))
    return bad
