"""K24 (s2m2_tsdf_integrate / s2m2_tsdf_extract: depth maps fused into a TSDF volume, and its surface points) against the same results composed
from torch ops, same box, same process, alternated.

Integrate: B = 1 and 4 frames of 1216x1024 into volumes of 256^3 and 512^3 voxels that span the view at 2 m, for a plane at 2 m (`plane`) and
for two surfaces at 1.5 m and 2.5 m side by side (`two`), with carve 0 and 1.  The torch composition is the header's formulas as whole-volume
tensor ops -- the projection, three gathers from the maps and three from the image, and `torch.where` over every field -- frame by frame; its
result is compared with K24's before anything is timed: the voxels whose weight differs, and among the others those whose colour differs
and the largest tsdf difference.  (torch's device arithmetic is not the header's bit for bit: where 100 / disp is not exact, as for the 1.5 m surface of
`two`, its tsdf differs in the last bits (measured); the voxels with another weight appear only in that scene, which fits a voxel
whose sdf sits on a band edge falling on the other side of it -- whole slices of a grid that is aligned with the surface -- but that
cause is supposed, not shown.  K24 itself is pinned bit for bit by
tests/test_hip_tsdf.py against the numpy oracle.)  The timed calls go on fusing
the same frames into the same volume (the weights run up to the cap of 64; the voxels a call updates do not change), and neither side is
charged a clear.  K24 is timed with events around `--steps` replays of a hipGraph that holds one call; the composition with events around
`--torch-steps` eager calls after a warm-up call, in the same alternated windows.  Figures are the median of `--repeats` windows with minimum
and maximum.

TRAFFIC: a voxel that a call updates is read and written once: 32 bytes.  `updated x 32 B / time` is the rate at which K24 moves the voxels
it has to move, printed as a share of the HBM rate a float4 copy reaches on this part (6.29 TB/s; 8.0 TB/s is the specification).  It is NOT the
kernel's whole traffic: every voxel is also projected and gathers three map values per frame whether or not it is updated, which the figure
leaves out, so a low share with carve 0 says that the launch is bound by the voxels it skips.

Extract: the surface points of the volumes above after the B = 4 call, against nonzero + gathers in torch (which synchronises to size its
result); the counts are compared.

    python tools/tsdfbench.py [--steps 20] [--torch-steps 3] [--repeats 5] [--forward] [--dims 256,512] [--mesh | --raycast | --track] [--out FILE]

--mesh (K25, s2m2_tsdf_mesh; default --out profiles/tsdf/tsdfmesh.txt) measures the triangle mesh instead, on the same volumes (the B = 4, carve 1
call of each scene, fused once): K25, s2m2_tsdf_extract alone on the same volume (what the triangles cost on top of the vertices), and the same
faces composed from torch ops -- the case index from eight shifted comparisons, a gather from the case table, `nonzero` over the cells, and the
rank map by a `cumsum` over the emit flags -- which is what a user can do today without K25.  The composition's faces are compared with K25's
once per volume, at the timed size.  MANDATORY BYTES of K25: the volume read once (16 B per voxel) plus the outputs written (16 + 12 B per vertex,
12 B per face); over the time they are printed as a share of the same 6.29 TB/s copy rate.  K25 reads the volume in each of its three launches and
writes and reads a rank map of 4 B per voxel, which the figure leaves out on purpose: it is the traffic a perfect kernel would need.

--raycast (K26, s2m2_tsdf_raycast; default --out profiles/tsdf/tsdfraycast.txt) measures the ray caster on the same volumes: depth, gradients,
image and count at 640x480 and 1216x1024 from two poses (the first frame's, and one turned by 0.2 rad about y), with the API's defaults (z_near
0, z_far the farthest corner of the grid, step trunc / 2).  Against it: the same maps composed from torch ops -- a march of `grid_sample` over
the tsdf and the observed flag with the same step, which keeps K26's state (have_prev, t_prev, z_prev) as whole-image tensors, takes every one
of the n_steps samples for every pixel (leaving early would need a synchronisation per step) and samples the hit again for depth and gradient;
compared with K26 on the pixels both cover (torch's arithmetic is not the rule's bit for bit: a sample on a cell face or beside an unobserved
voxel may take another cell or another step, which shows as a few pixels covered by one side only and as a whole-cell change of a gradient) -- and s2m2_tsdf_extract on the same volume, which is what a user pays today before a rasteriser
on the host.  GATHERED BYTES: a sample inside the grid reads 8 voxels x 8 B = 64 B; the samples a ray takes inside the grid up to its hit are
counted by the torch march (K26's own clip may take a few more at the box's faces), and samples x 64 B over K26's time is printed as a share of
the 6.29 TB/s copy rate.  Neighbouring rays share most of those bytes in the caches, so the figure is the gather rate, not HBM traffic.

--track (K27, s2m2_tsdf_track; default --out profiles/tsdf/tsdftrack.txt) measures the tracker: a curved surface around 2 m fused once at the
identity into the 256^3 and 512^3 volumes, K26's depth and gradient maps of it at 640x480 and 1216x1024 from the identity, and live frames of
1216x1024 and 640x480 of the same surface, tracked from a pose 0.01 rad and 1 cm off.  Timed as hipGraph replays: the call of 10 iterations (per
iteration: a tenth; per launch: a twentieth -- the MEAN of the sums launch and the solve launch, which this tool cannot tell apart; the kernel
trace of a profiler run can), and the chain raycast + track + integrate of one frame; both also as a share of an S forward at 1216x1024 (7.97
ms).  The replays go on from the pose the call before left, i.e. at the converged pose, where the work is the same.  MANDATORY BYTES per
iteration: the three live maps read once (12 B per live pixel) plus 16 B (depth and three gradient planes) per live pixel that lands inside
the model image; over the time of an iteration they are printed as a share of the 6.29 TB/s copy rate.  Beside it: the same 28 sums and the
count composed from torch ops -- the per-pixel rule as whole-image fp32 tensors, four gathers, and J^T J as one float64 matmul -- compared
with K27's first row of `systems` (torch's arithmetic is not the rule's bit for bit; a pixel on the gate's edge may fall on the other side).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1024, 1216
CAM = dict(fx=1000.0, fy=1000.0, cx=608.0, cy=512.0, baseline=100.0, doffs=0.0, depth_scale=1000.0, depth_trunc=10.0, conf_min=0.1, occ_min=0.5)
HBM_COPY_TBS = 6.29


def torch_integrate(torch, vol, disp, occ, conf, img, poses, origin, vs, trunc, max_weight, carve):
    """the header's formulas over the whole volume, pair by pair; vol (Nz,Ny,Nx,4) int32 is updated in place"""
    Nz, Ny, Nx, _ = vol.shape
    dev = vol.device
    f32 = torch.float32
    x = (origin[0] + torch.arange(Nx, device=dev, dtype=f32) * vs)[None, None, :]
    y = (origin[1] + torch.arange(Ny, device=dev, dtype=f32) * vs)[None, :, None]
    z = (origin[2] + torch.arange(Nz, device=dev, dtype=f32) * vs)[:, None, None]
    tsdf, weight = vol[..., 0].view(f32).clone(), vol[..., 1].clone()
    col = [vol[..., 2] & 0xffff, (vol[..., 2] >> 16) & 0xffff, vol[..., 3] & 0xffff]
    pad = vol[..., 3] & ~0xffff
    bf = CAM["baseline"] * CAM["fx"]
    for b in range(disp.shape[0]):
        q = poses[b].tolist()
        X = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
        Y = ((q[4] * x + q[5] * y) + q[6] * z) + q[7]
        Z = ((q[8] * x + q[9] * y) + q[10] * z) + q[11]
        fu = torch.round((CAM["fx"] * X) / Z + CAM["cx"])
        fv = torch.round((CAM["fy"] * Y) / Z + CAM["cy"])
        inside = (Z > 0) & torch.isfinite(Z) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        pix = torch.where(inside, fv * W + fu, 0.0).long().reshape(-1)
        d = disp[b, 0].reshape(-1)[pix].reshape(Z.shape)
        valid = (conf[b, 0].reshape(-1)[pix].reshape(Z.shape) > CAM["conf_min"]) & (occ[b, 0].reshape(-1)[pix].reshape(Z.shape) > CAM["occ_min"])
        d = torch.where(valid, d, -1.0)
        zp = torch.where(d <= 0, 1e9, bf / (d + CAM["doffs"])) / CAM["depth_scale"]
        keep = inside & (zp > 0) & (zp < CAM["depth_trunc"])
        sdf = zp - Z
        upd = keep & (sdf >= -trunc)
        if not carve:
            upd &= ~(sdf > trunc)
        dd = torch.clamp_max(sdf / trunc, 1.0)
        Wf = weight.float()
        tsdf = torch.where(upd, (tsdf * Wf + dd) / (Wf + 1.0), tsdf)
        for ch in range(3):
            byte = img[b, ch].reshape(-1)[pix].reshape(Z.shape).int()
            new = (col[ch].long() * weight + (byte << 8) + ((weight + 1) >> 1)) // (weight + 1)
            col[ch] = torch.where(upd, new.int(), col[ch])
        weight = torch.where(upd, torch.clamp_max(weight + 1, max_weight), weight)
    vol[..., 0] = tsdf.view(torch.int32)
    vol[..., 1] = weight
    vol[..., 2] = col[0] | (col[1] << 16)
    vol[..., 3] = col[2] | pad


def torch_extract(torch, vol, origin, vs, min_weight):
    """the surface points from nonzero + gathers -> (xyz (n,3) fp32, rgb (n,3) uint8, gradients (n,3) fp32); points run by axis, then by
    voxel (K24 runs by voxel, then by axis: the same set)"""
    Nz, Ny, Nx, _ = vol.shape
    f32 = torch.float32
    t, obs = vol[..., 0].view(f32), vol[..., 1] >= min_weight
    colour = torch.stack([vol[..., 2] & 0xffff, (vol[..., 2] >> 16) & 0xffff, vol[..., 3] & 0xffff], -1)
    tpad = torch.nn.functional.pad(torch.where(obs, t, float("nan")), (1, 1, 1, 1, 1, 1), value=float("nan"))      # NaN: outside or unobserved
    out = []
    for a, dim in enumerate((2, 1, 0)):                                # x, y, z are the tensor dims 2, 1, 0
        n = vol.shape[dim]
        t0, t1 = t.narrow(dim, 0, n - 1), t.narrow(dim, 1, n - 1)
        emit = obs.narrow(dim, 0, n - 1) & obs.narrow(dim, 1, n - 1) & ((t0 < 0) != (t1 < 0))
        idx = torch.nonzero(emit)                                      # synchronises
        k, j, i = idx[:, 0], idx[:, 1], idx[:, 2]
        a0, a1 = t0[k, j, i], t1[k, j, i]
        s = a0 / (a0 - a1)
        xyz = torch.stack([origin[0] + i.float() * vs, origin[1] + j.float() * vs, origin[2] + k.float() * vs], 1)
        xyz[:, a] = xyz[:, a] + s * vs
        far = (a1.abs() < a0.abs()).long()
        sel = [k + far * (dim == 0), j + far * (dim == 1), i + far * (dim == 2)]
        rgb = ((colour[sel[0], sel[1], sel[2]] + 128) >> 8).to(torch.uint8)
        ts = torch.where(far.bool(), a1, a0)
        grad = []
        for off in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
            tp = tpad[sel[0] + 1 + off[0], sel[1] + 1 + off[1], sel[2] + 1 + off[2]]
            tm = tpad[sel[0] + 1 - off[0], sel[1] + 1 - off[1], sel[2] + 1 - off[2]]
            grad.append(torch.where(torch.isnan(tp), ts, tp) - torch.where(torch.isnan(tm), ts, tm))
        out.append((xyz, rgb, torch.stack(grad, 1)))
    return tuple(torch.cat([o[c] for o in out]) for c in range(3))


def mesh_tables(torch, device="cuda"):
    """the case table of s2m2_amd/mc_table.py as device tensors: triangles per case (256), their edges (256, 5, 3), and per edge its axis and the
    offset (dz, dy, dx) of its base corner"""
    from s2m2_amd import mc_table
    table = mc_table.build_table()
    most = mc_table.max_triangles(table)
    count = torch.tensor([len(t) for t in table], device=device, dtype=torch.int64)
    edges = torch.zeros((256, most, 3), device=device, dtype=torch.int64)
    for case, tris in enumerate(table):
        for n, tri in enumerate(tris):
            edges[case, n] = torch.tensor(tri)
    axis = torch.tensor([a for a, _ in mc_table.EDGES], device=device, dtype=torch.int64)
    base = torch.tensor([[b >> 2, b >> 1 & 1, b & 1] for _, b in mc_table.EDGES], device=device, dtype=torch.int64)
    return count, edges, axis, base


def torch_mesh_faces(torch, vol, min_weight, tables):
    """K25's faces from torch ops -> (m, 3) int32 vertex ranks, in K25's order"""
    count, edges, axis, base = tables
    Nz, Ny, Nx, _ = vol.shape
    t, obs = vol[..., 0].view(torch.float32), vol[..., 1] >= min_weight
    neg = t < 0
    case = torch.zeros((Nz - 1, Ny - 1, Nx - 1), device=vol.device, dtype=torch.int64)
    valid = torch.ones_like(case, dtype=torch.bool)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2
        case |= neg[dz:Nz - 1 + dz, dy:Ny - 1 + dy, dx:Nx - 1 + dx].long() << c
        valid &= obs[dz:Nz - 1 + dz, dy:Ny - 1 + dy, dx:Nx - 1 + dx]
    emit = torch.zeros((Nz, Ny, Nx, 3), device=vol.device, dtype=torch.int32)
    emit[:, :, :-1, 0] = obs[:, :, :-1] & obs[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    emit[:, :-1, :, 1] = obs[:, :-1] & obs[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    emit[:-1, :, :, 2] = obs[:-1] & obs[1:] & (neg[:-1] != neg[1:])
    flat = emit.reshape(-1)
    rank = torch.cumsum(flat, 0, dtype=torch.int32) - flat                # (voxel, axis) -> the rank of its point
    per_cell = torch.where(valid, count[case], 0)
    cells = torch.nonzero(per_cell)                                       # synchronises; ascending lin
    k, j, i = cells[:, 0], cells[:, 1], cells[:, 2]
    cs, per = case[k, j, i], per_cell[k, j, i]
    which = torch.repeat_interleave(torch.arange(len(cs), device=vol.device), per)
    tri = torch.arange(len(which), device=vol.device) - torch.repeat_interleave(torch.cumsum(per, 0) - per, per)
    e = edges[cs[which], tri]                                             # (m, 3) edge numbers
    off = base[e]                                                         # (m, 3, 3)
    voxel = ((k[which, None] + off[..., 0]) * Ny + j[which, None] + off[..., 1]) * Nx + i[which, None] + off[..., 2]
    return rank[voxel * 3 + axis[e]]


def mesh_main(a, torch, hip, say) -> None:
    from tools.kbench import captured, spread, timed
    tables = mesh_tables(torch)
    g = torch.Generator(device="cuda").manual_seed(7)
    vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    depth = dict(plane=torch.full((H, W), 2.0, device="cuda"), two=torch.where(uu < W // 2, 1.5, 2.5))
    one = torch.ones((4, 1, H, W), device="cuda")
    img = torch.randint(0, 256, (4, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
    poses = torch.tensor([[1, 0, 0, 0.01 * b, 0, 1, 0, -0.005 * b, 0, 0, 1, 0.02 * b] for b in range(4)], device="cuda", dtype=torch.float32)
    for N in (int(x) for x in a.dims.split(",")):
        vs = 2.048 / N
        origin, trunc = (-1.024 + vs / 2, -1.024 + vs / 2, 1.0), 4 * vs
        place = dict(origin=origin, voxel_size=vs)
        ws = torch.empty(hip.tsdf_workspace_bytes(N, N, N), device="cuda", dtype=torch.uint8)
        mws = torch.empty(hip.tsdf_mesh_workspace_bytes(N, N, N), device="cuda", dtype=torch.uint8)
        cap = N * N * N // 4
        rec = torch.empty((cap, 4), device="cuda", dtype=torch.int32)
        grd = torch.empty((cap, 3), device="cuda", dtype=torch.float32)
        cnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
        faces = torch.empty((2 * cap, 3), device="cuda", dtype=torch.int32)
        fcnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
        for scene, z in depth.items():
            disp = (100.0 / z)[None, None].repeat(4, 1, 1, 1).contiguous()
            vol = torch.zeros((N, N, N, 4), device="cuda", dtype=torch.int32)
            hip.tsdf_integrate(vol, disp, one, one, img, poses, **CAM, **place, trunc=trunc, max_weight=64, carve=True)
            mesh = lambda: hip.tsdf_mesh(vol, **place, min_weight=1, workspace=mws, records=rec, gradients=grd, count=cnt, faces=faces, face_count=fcnt)      # noqa: E731
            extract = lambda: hip.tsdf_extract(vol, **place, min_weight=1, workspace=ws, records=rec, gradients=grd, count=cnt)      # noqa: E731
            compose = lambda: torch_mesh_faces(torch, vol, 1, tables)      # noqa: E731
            mesh()
            n, nf = int(cnt[0]), int(fcnt[0])
            ref = compose()
            equal = nf <= len(faces) and ref.shape[0] == nf and bool((ref == faces[:nf]).all())
            del ref
            gm, gx = captured(mesh), captured(extract)
            tm, tx, tt = [], [], []
            for _ in range(a.repeats):
                tm.append(timed(gm.replay, a.steps))
                tx.append(timed(gx.replay, a.steps))
                tt.append(timed(compose, a.torch_steps))
            um, ux, ut = statistics.median(tm), statistics.median(tx), statistics.median(tt)
            mandatory = N ** 3 * 16 + n * 28 + nf * 12 + 8
            say(f"mesh      {N}^3 {scene:5s}: {n} vertices, {nf} faces (torch composition's faces equal K25's: {equal}), capacities {cap} / {2 * cap}")
            say(f"    K25                {spread(tm)}   {mandatory} mandatory bytes = {mandatory / um / 1e6:6.3f} TB/s = "
                f"{mandatory / um / 1e6 / HBM_COPY_TBS * 100:5.1f} % of the {HBM_COPY_TBS} TB/s copy rate")
            say(f"    K24 extract alone  {spread(tx)}   K25 = {um / ux:5.2f}x the vertices alone")
            say(f"    torch composition  {spread(tt)}   {ut / um:6.1f}x K25 (faces only: it computes no vertex)")
            del gm, gx, vol


def torch_raycast(torch, tsdf, obs, pose, Ht, Wt, fx, fy, cx, cy, origin, vs, z_near, step, n_steps):
    """K26's rule from torch ops: tsdf, obs (1,1,Nz,Ny,Nx) fp32 (obs: 1.0 where weight >= min_weight) -> depth (Ht,Wt), gradient (3,Ht,Wt) and
    the number of samples taken inside the grid while a ray was still marching (a device scalar)"""
    Nz, Ny, Nx = tsdf.shape[2:]
    dev = tsdf.device
    q = pose.tolist()
    v, u = torch.meshgrid(torch.arange(Ht, device=dev, dtype=torch.float32), torch.arange(Wt, device=dev, dtype=torch.float32), indexing="ij")
    dx, dy = (u - cx) / fx, (v - cy) / fy
    a = [(-(q[c] * q[3] + q[4 + c] * q[7] + q[8 + c] * q[11]) - origin[c]) / vs for c in range(3)]
    b = [(q[c] * dx + q[4 + c] * dy + q[8 + c]) / vs for c in range(3)]
    top = (Nx - 1, Ny - 1, Nz - 1)

    def sample(z):
        g = [a[c] + z * b[c] for c in range(3)]
        inside = (g[0] >= 0) & (g[0] < top[0]) & (g[1] >= 0) & (g[1] < top[1]) & (g[2] >= 0) & (g[2] < top[2])
        grid = torch.stack([2.0 * g[c] / top[c] - 1.0 for c in range(3)], -1)[None, None]           # (1,1,Ht,Wt,3): x, y, z
        t = torch.nn.functional.grid_sample(tsdf, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
        o = torch.nn.functional.grid_sample(obs, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
        return inside, inside & (o > 0.999999), t, g

    have = torch.zeros((Ht, Wt), device=dev, dtype=torch.bool)
    done = torch.zeros_like(have)
    t_prev, z_prev, t_hit, z_at = (torch.zeros((Ht, Wt), device=dev) for _ in range(4))
    samples = torch.zeros((), device=dev, dtype=torch.int64)
    for k in range(n_steps):
        z = z_near + k * step
        inside, ok, t, _ = sample(z)
        live = ~done
        samples += (live & inside).sum()
        cross = live & ok & have & ~(t_prev < 0) & (t < 0)
        t_hit = torch.where(cross, t, t_hit)
        z_at = torch.where(cross, z, z_at)
        done |= cross
        go = live & ok & ~cross
        have = torch.where(live, ok & ~cross, have)
        t_prev = torch.where(go, t, t_prev)
        z_prev = torch.where(go, z, z_prev)
    z_hit = z_prev + (t_prev / (t_prev - t_hit)) * (z_at - z_prev)
    z_hit = torch.where(done, z_hit, 0.0)
    _, ok, _, g = sample(z_hit)
    covered = done & ok
    grad = []
    for c in range(3):                                      # the interpolant is linear along each axis inside a cell: its slope from the cell's two faces
        lo, hi = list(g), list(g)
        lo[c] = torch.floor(g[c])
        hi[c] = lo[c] + 1.0
        gl = torch.stack([2.0 * lo[d] / top[d] - 1.0 for d in range(3)], -1)[None, None]
        gh = torch.stack([2.0 * hi[d] / top[d] - 1.0 for d in range(3)], -1)[None, None]
        tl = torch.nn.functional.grid_sample(tsdf, gl, mode="bilinear", padding_mode="border", align_corners=True)[0, 0, 0]
        th = torch.nn.functional.grid_sample(tsdf, gh, mode="bilinear", padding_mode="border", align_corners=True)[0, 0, 0]
        grad.append(torch.where(covered, th - tl, 0.0))
    return torch.where(covered, z_hit, 0.0), torch.stack(grad), samples


def raycast_main(a, torch, hip, say) -> None:
    import math
    from tools.kbench import captured, spread, timed
    g = torch.Generator(device="cuda").manual_seed(7)
    vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    depth = dict(plane=torch.full((H, W), 2.0, device="cuda"), two=torch.where(uu < W // 2, 1.5, 2.5))
    one = torch.ones((4, 1, H, W), device="cuda")
    img = torch.randint(0, 256, (4, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
    poses = torch.tensor([[1, 0, 0, 0.01 * b, 0, 1, 0, -0.005 * b, 0, 0, 1, 0.02 * b] for b in range(4)], device="cuda", dtype=torch.float32)
    c2, s2 = math.cos(0.2), math.sin(0.2)
    views = dict(front=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], turned=[c2, 0, s2, -2 * s2, 0, 1, 0, 0, -s2, 0, c2, 2 - 2 * c2])     # turned about (0, 0, 2)
    for N in (int(x) for x in a.dims.split(",")):
        vs = 2.048 / N
        origin, trunc = (-1.024 + vs / 2, -1.024 + vs / 2, 1.0), 4 * vs
        place = dict(origin=origin, voxel_size=vs)
        ws = torch.empty(hip.tsdf_workspace_bytes(N, N, N), device="cuda", dtype=torch.uint8)
        cap = N * N * N // 4
        rec = torch.empty((cap, 4), device="cuda", dtype=torch.int32)
        grd = torch.empty((cap, 3), device="cuda", dtype=torch.float32)
        cnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
        for scene, z in depth.items():
            disp = (100.0 / z)[None, None].repeat(4, 1, 1, 1).contiguous()
            vol = torch.zeros((N, N, N, 4), device="cuda", dtype=torch.int32)
            hip.tsdf_integrate(vol, disp, one, one, img, poses, **CAM, **place, trunc=trunc, max_weight=64, carve=True)
            tsdf = vol[..., 0].view(torch.float32)[None, None].contiguous()
            obs = (vol[..., 1] >= 1).float()[None, None].contiguous()
            extract = lambda: hip.tsdf_extract(vol, **place, min_weight=1, workspace=ws, records=rec, gradients=grd, count=cnt)      # noqa: E731
            extract()
            gx = captured(extract)
            tx = [timed(gx.replay, a.steps) for _ in range(a.repeats)]
            say(f"raycast   {N}^3 {scene:5s}: voxel {vs * 1000:.0f} mm, step {trunc / 2 * 1000:.0f} mm; K24 extract of the volume ({int(cnt[0])} points) {spread(tx)}")
            for (Wt, Ht) in ((640, 480), (W, H)):
                k = Wt / W
                cam = dict(fx=CAM["fx"] * k, fy=CAM["fy"] * k, cx=CAM["cx"] * k, cy=CAM["cy"] * Ht / H)
                for view, pose in views.items():
                    pb = torch.tensor([pose], device="cuda", dtype=torch.float32)
                    qd = [float(x) for x in pose]
                    centre = [-(qd[c] * qd[3] + qd[4 + c] * qd[7] + qd[8 + c] * qd[11]) for c in range(3)]
                    z_far = max(math.dist(centre, [origin[c] + (N - 1) * vs * ((corner >> c) & 1) for c in range(3)]) for corner in range(8))
                    n_steps = hip.tsdf_raycast_steps(0.0, z_far, trunc / 2)
                    out = dict(depth=torch.empty((1, 1, Ht, Wt), device="cuda"), gradients=torch.empty((1, 3, Ht, Wt), device="cuda"),
                               image=torch.empty((1, 3, Ht, Wt), device="cuda", dtype=torch.uint8), count=torch.zeros((1,), device="cuda", dtype=torch.int32))
                    cast = lambda: hip.tsdf_raycast(vol, pb, Ht=Ht, Wt=Wt, **cam, **place, min_weight=1, z_near=0.0, z_far=z_far, step=trunc / 2, **out)      # noqa: E731
                    compose = lambda: torch_raycast(torch, tsdf, obs, pb[0], Ht, Wt, cam["fx"], cam["fy"], cam["cx"], cam["cy"], origin, vs, 0.0, trunc / 2, n_steps)      # noqa: E731
                    cast()
                    td, tg, samples = compose()
                    kd, covered = out["depth"][0, 0], int(out["count"][0])
                    both = (kd != 0) & (td != 0)
                    err = float((kd - td)[both].abs().max()) if bool(both.any()) else float("nan")
                    gerr = float((out["gradients"][0] - tg)[:, both].abs().max()) if bool(both.any()) else float("nan")
                    samples = int(samples)
                    gk = captured(cast)
                    tk, tt = [], []
                    for _ in range(a.repeats):
                        tk.append(timed(gk.replay, a.steps))
                        tt.append(timed(compose, a.torch_steps))
                    uk, ut, ux = statistics.median(tk), statistics.median(tt), statistics.median(tx)
                    say(f"  {Wt}x{Ht} {view:6s}: {n_steps} steps, {covered} of {Ht * Wt} pixels covered (torch: {int((td != 0).sum())}; both {int(both.sum())}, "
                        f"max |depth difference| {err:.2e}, max |gradient difference| {gerr:.2e})")
                    say(f"    K26                {spread(tk)}   {samples / (Ht * Wt):6.1f} samples per ray inside the grid x 64 B = {samples * 64 / 1e6:8.1f} MB gathered = "
                        f"{samples * 64 / uk / 1e6:6.3f} TB/s = {samples * 64 / uk / 1e6 / HBM_COPY_TBS * 100:5.1f} % of the {HBM_COPY_TBS} TB/s copy rate")
                    say(f"    torch composition  {spread(tt)}   {ut / uk:6.1f}x K26")
                    say(f"    K24 extract        {ux:8.1f} us            {ux / uk:6.2f}x K26" + ("   (extract is faster)" if ux < uk else ""))
                    del gk
            del gx, vol, tsdf, obs


FORWARD_MS = 7.97                                        # an S forward at 1216x1024 fp16 (profiles/: the flagship measurement)


def torch_track_sums(torch, disp, pose, mpose, md, mg, cam, mcam, max_dist):
    """one iteration's sums of K27 from torch ops: disp (H,W), md (Ht,Wt), mg (3,Ht,Wt) -> (sums (28) float64, count, live pixels inside the
    model image)"""
    Hl, Wl = disp.shape
    Ht, Wt = md.shape
    dev = disp.device
    q, m = pose.tolist(), mpose.tolist()
    v, u = torch.meshgrid(torch.arange(Hl, device=dev, dtype=torch.float32), torch.arange(Wl, device=dev, dtype=torch.float32), indexing="ij")
    z = torch.where(disp <= 0, 1e9, (cam["baseline"] * cam["fx"]) / (disp + cam["doffs"])) / cam["depth_scale"]
    keep = (z > 0) & (z < cam["depth_trunc"])
    x, y = (u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"]
    c = (x - q[3], y - q[7], z - q[11])
    p = [q[a] * c[0] + q[4 + a] * c[1] + q[8 + a] * c[2] for a in range(3)]
    X, Y, Z = (m[4 * r] * p[0] + m[4 * r + 1] * p[1] + m[4 * r + 2] * p[2] + m[4 * r + 3] for r in range(3))
    fu, fv = torch.round(mcam["fx"] * X / Z + mcam["cx"]), torch.round(mcam["fy"] * Y / Z + mcam["cy"])
    inside = keep & (Z > 0) & torch.isfinite(Z) & (fu >= 0) & (fu < Wt) & (fv >= 0) & (fv < Ht)
    pix = torch.where(inside, fv * Wt + fu, 0.0).long().reshape(-1)
    dm = md.reshape(-1)[pix].reshape(Z.shape)
    g = [mg[a].reshape(-1)[pix].reshape(Z.shape) for a in range(3)]
    s = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
    n = [ga / torch.sqrt(s) for ga in g]
    e = ((fu - mcam["cx"]) * dm / mcam["fx"] - m[3], (fv - mcam["cy"]) * dm / mcam["fy"] - m[7], dm - m[11])
    w = [m[a] * e[0] + m[4 + a] * e[1] + m[8 + a] * e[2] for a in range(3)]
    d = [w[a] - p[a] for a in range(3)]
    used = inside & (dm > 0) & (s > 0) & torch.isfinite(s) & (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= max_dist * max_dist)
    r = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    J = torch.stack([p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2], r], -1)
    J = torch.where(used[..., None], J, 0.0).reshape(-1, 7).double()
    A = J.T @ J
    iu = torch.triu_indices(6, 6, device=dev)
    return torch.cat([A[iu[0], iu[1]], A[:6, 6], A[6:, 6]]), used.sum(), inside.sum()


def track_main(a, torch, hip, say) -> None:
    import math
    from tools.kbench import captured, spread, timed
    n_iters = 10
    c1, s1 = math.cos(0.01), math.sin(0.01)
    start = [c1, 0, s1, 0.01, 0, 1, 0, -0.005, -s1, 0, c1, 0.005]                     # 0.01 rad about y and about 1 cm off the true pose
    ident = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], device="cuda", dtype=torch.float32)

    def frame(Wl, Hl):
        """the live maps of the curved surface at Wl x Hl and its camera"""
        k = Wl / W
        cam = dict(CAM, fx=CAM["fx"] * k, fy=CAM["fy"] * k, cx=CAM["cx"] * k, cy=CAM["cy"] * Hl / H)
        v, u = torch.meshgrid(torch.arange(Hl, device="cuda", dtype=torch.float32), torch.arange(Wl, device="cuda", dtype=torch.float32), indexing="ij")
        U, V = CAM["cx"] + (u - cam["cx"]) / k, CAM["cy"] + (v - cam["cy"]) / k        # the pixel of the 1216 x 1024 frame on the same ray
        z = 2.0 + 0.15 * torch.sin(U / 90.0) + 0.12 * torch.cos(V / 70.0) + 0.1 * torch.sin((U + V) / 110.0)
        return (cam["baseline"] * cam["fx"] / 1000.0 / z)[None, None].contiguous(), cam

    frames = {size: frame(*size) for size in ((W, H), (640, 480))}
    one = {size: torch.ones((1, 1, size[1], size[0]), device="cuda") for size in frames}
    img = {size: torch.zeros((1, 3, size[1], size[0]), device="cuda", dtype=torch.uint8) for size in frames}
    for N in (int(x) for x in a.dims.split(",")):
        vs = 2.048 / N
        origin, trunc = (-1.024 + vs / 2, -1.024 + vs / 2, 1.0), 4 * vs
        place = dict(origin=origin, voxel_size=vs)
        vol = torch.zeros((N, N, N, 4), device="cuda", dtype=torch.int32)
        disp0, cam0 = frames[(W, H)]
        hip.tsdf_integrate(vol, disp0, one[(W, H)], one[(W, H)], img[(W, H)], ident, **cam0, **place, trunc=trunc, max_weight=64, carve=True)
        z_far = max(math.dist([0, 0, 0], [origin[c] + (N - 1) * vs * ((corner >> c) & 1) for c in range(3)]) for corner in range(8))
        say(f"track     {N}^3: voxel {vs * 1000:.0f} mm, max_dist = trunc = {trunc * 1000:.0f} mm, {n_iters} iterations, start 0.01 rad / 12 mm off")
        for (Wt, Ht) in ((640, 480), (W, H)):
            mcam = {k: frames[(Wt, Ht)][1][k] for k in ("fx", "fy", "cx", "cy")}
            md = torch.empty((1, 1, Ht, Wt), device="cuda")
            mg = torch.empty((1, 3, Ht, Wt), device="cuda")
            cast = lambda pb: hip.tsdf_raycast(vol, pb, Ht=Ht, Wt=Wt, **mcam, **place, min_weight=1, z_near=0.0, z_far=z_far, step=trunc / 2, depth=md, gradients=mg)      # noqa: E731
            cast(ident)
            for (Wl, Hl) in ((W, H), (640, 480)):
                disp, cam = frames[(Wl, Hl)]
                maps = (disp, one[(Wl, Hl)], one[(Wl, Hl)])
                ws = torch.empty(hip.tsdf_track_workspace_bytes(1, Hl, Wl) // 8, device="cuda", dtype=torch.float64)
                pb = torch.tensor([start], device="cuda", dtype=torch.float32)
                systems = torch.zeros((1, n_iters, 32), device="cuda", dtype=torch.float64)
                kw = dict(H=Hl, W=Wl, **cam, mfx=mcam["fx"], mfy=mcam["fy"], mcx=mcam["cx"], mcy=mcam["cy"], max_dist=trunc, min_count=100, max_rot=0.2,
                          max_trans=4 * trunc, workspace=ws)
                track = lambda: hip.tsdf_track(*maps, pb, ident, md, mg, n_iters=n_iters, systems=systems, **kw)      # noqa: E731
                mp = ident.clone()

                def chain():
                    mp.copy_(pb)
                    cast(mp)
                    hip.tsdf_track(*maps, pb, mp, md, mg, n_iters=n_iters, systems=systems, **kw)
                    hip.tsdf_integrate(vol, *maps, img[(Wl, Hl)], pb, **cam, **place, trunc=trunc, max_weight=64, carve=True)

                compose = lambda: torch_track_sums(torch, disp[0, 0], torch.tensor(start), ident[0].cpu(), md[0, 0], mg[0], cam, mcam, trunc)      # noqa: E731
                track()
                first = systems[0, 0].cpu()
                statuses = systems[0, :, 29].int().tolist()
                ts, tc, tin = compose()
                rel = float(((ts.cpu() - first[:28]).abs() / first[:28].abs().clamp_min(1e-30)).max())
                t_rot, t_tr = float(torch.arccos(((pb[0, 0] + pb[0, 5] + pb[0, 10] - 1) / 2).clamp(-1, 1))), float(pb[0, [3, 7, 11]].norm())
                gt = captured(track)
                tk, tt = [], []
                for _ in range(a.repeats):
                    tk.append(timed(gt.replay, a.steps))
                    tt.append(timed(compose, a.torch_steps))
                del gt
                cast(ident)
                pb.copy_(torch.tensor([start], device="cuda"))
                keep = vol.clone()                                               # the chain fuses a frame per replay: timed on a volume of its own
                gc = captured(chain)
                tch = [timed(gc.replay, a.steps) for _ in range(a.repeats)]
                del gc
                vol.copy_(keep)
                del keep
                cast(ident)
                uk, ut, uc = statistics.median(tk), statistics.median(tt), statistics.median(tch)
                mandatory = 12 * Hl * Wl + 16 * int(tin)
                say(f"  live {Wl}x{Hl} against model {Wt}x{Ht}: {int(first[28])} correspondences of {Hl * Wl} pixels in the first iteration (torch: {int(tc)}, "
                    f"largest relative difference of a sum {rel:.1e}); statuses {statuses}; left {t_rot:.1e} rad, {t_tr * 1000:.2f} mm from the true pose")
                say(f"    K27, {n_iters} iterations  {spread(tk)}   {uk / n_iters:7.1f} us per iteration, {uk / n_iters / 2:6.1f} us per launch (mean of two)   "
                    f"{uk / FORWARD_MS / 10:.2f} % of an S forward ({FORWARD_MS} ms)")
                say(f"    mandatory bytes per iteration {mandatory} = {mandatory / (uk / n_iters) / 1e6:6.3f} TB/s = "
                    f"{mandatory / (uk / n_iters) / 1e6 / HBM_COPY_TBS * 100:5.1f} % of the {HBM_COPY_TBS} TB/s copy rate")
                say(f"    torch composition of one iteration's sums  {spread(tt)}   {ut / (uk / n_iters):6.1f}x an iteration of K27" +
                    ("   (torch is faster)" if ut < uk / n_iters else ""))
                say(f"    raycast + track + integrate  {spread(tch)}   {uc / FORWARD_MS / 10:.2f} % of an S forward")
        del vol


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--dims", default="256,512")
    ap.add_argument("--mesh", action="store_true", help="measure K25 (the triangle mesh) instead; default --out profiles/tsdf/tsdfmesh.txt")
    ap.add_argument("--raycast", action="store_true", help="measure K26 (the ray caster) instead; default --out profiles/tsdf/tsdfraycast.txt")
    ap.add_argument("--track", action="store_true", help="measure K27 (the tracker) instead; default --out profiles/tsdf/tsdftrack.txt")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tsdf",
                             "tsdftrack.txt" if a.track else "tsdfraycast.txt" if a.raycast else "tsdfmesh.txt" if a.mesh else "tsdfbench.txt")
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    if a.mesh or a.raycast or a.track:
        (track_main if a.track else raycast_main if a.raycast else mesh_main)(a, torch, hip, say)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return

    forward_us = None
    if a.forward:
        from s2m2_amd.model import build_model
        from s2m2_amd.spec import MODEL_CONFIGS
        from s2m2_amd.weights import seeded_state_dict, synthetic_pair
        C, ntr = MODEL_CONFIGS["S"]
        m = build_model("S")
        m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
        m = m.cuda().eval()
        l, r = (t.cuda().contiguous() for t in synthetic_pair(H, W, 1, 32, 0))
        with torch.autocast("cuda", dtype=torch.float16):
            for _ in range(3):
                m(l, r)
            forward_us = statistics.median(timed(lambda: m(l, r), 50) for _ in range(a.repeats))
        say(f"S forward {W}x{H} fp16 (hipGraph replay, same session): {forward_us / 1000.0:.3f} ms")
        del m

    g = torch.Generator(device="cuda").manual_seed(7)
    vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    depth = dict(plane=torch.full((H, W), 2.0, device="cuda"), two=torch.where(uu < W // 2, 1.5, 2.5))
    one = torch.ones((4, 1, H, W), device="cuda")
    img = torch.randint(0, 256, (4, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
    poses = torch.tensor([[1, 0, 0, 0.01 * b, 0, 1, 0, -0.005 * b, 0, 0, 1, 0.02 * b] for b in range(4)], device="cuda", dtype=torch.float32)
    for N in (int(x) for x in a.dims.split(",")):
        vs = 2.048 / N
        origin, trunc = (-1.024 + vs / 2, -1.024 + vs / 2, 1.0), 4 * vs
        place = dict(origin=origin, voxel_size=vs)
        ws = torch.empty(hip.tsdf_workspace_bytes(N, N, N), device="cuda", dtype=torch.uint8)
        for scene, z in depth.items():
            disp = (100.0 / z)[None, None].repeat(4, 1, 1, 1).contiguous()
            for B in (1, 4):
                for carve in (False, True):
                    maps = (disp[:B], one[:B], one[:B], img[:B], poses[:B])
                    kw = dict(**CAM, **place, trunc=trunc, max_weight=64, carve=carve)
                    vol = torch.zeros((N, N, N, 4), device="cuda", dtype=torch.int32)
                    ref = torch.zeros_like(vol)
                    hip.tsdf_integrate(vol, *maps, **kw)
                    torch_integrate(torch, ref, *maps, origin, vs, trunc, 64, carve)
                    torch.cuda.synchronize()
                    updated = int((vol[..., 1] > 0).sum())
                    same = vol[..., 1] == ref[..., 1]
                    diff_w = int((~same).sum())
                    err = float(torch.where(same, vol[..., 0].view(torch.float32) - ref[..., 0].view(torch.float32), 0.0).abs().max())
                    diff_c = int((same & (vol[..., 2:] != ref[..., 2:]).any(-1)).sum())
                    graph = captured(lambda: hip.tsdf_integrate(vol, *maps, **kw))
                    tk, tt = [], []
                    for _ in range(a.repeats):
                        tk.append(timed(graph.replay, a.steps))
                        tt.append(timed(lambda: torch_integrate(torch, ref, *maps, origin, vs, trunc, 64, carve), a.torch_steps))
                    uk, ut = statistics.median(tk), statistics.median(tt)
                    say(f"integrate {N}^3 {scene:5s} B={B} carve={int(carve)}: {updated} voxels updated of {N ** 3} "
                        f"(torch: {diff_w} voxels with another weight; among the others {diff_c} with another colour, max |tsdf difference| {err:.2e})")
                    say(f"    K24                {spread(tk)}   {updated * 32 / uk / 1e6:6.3f} TB/s of updated voxels = "
                        f"{updated * 32 / uk / 1e6 / HBM_COPY_TBS * 100:5.1f} % of the {HBM_COPY_TBS} TB/s copy rate" +
                        (f"   {uk / B / forward_us * 100:.2f} % of an S forward per frame" if forward_us else ""))
                    say(f"    torch composition  {spread(tt)}   {ut / uk:6.1f}x K24")
                    del graph
            # extraction of the last volume of the scene (B = 4, carve 1 on top of what the timing loops added)
            cap = N * N * N // 4
            rec = torch.empty((cap, 4), device="cuda", dtype=torch.int32)
            grd = torch.empty((cap, 3), device="cuda", dtype=torch.float32)
            cnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
            run = lambda: hip.tsdf_extract(vol, **place, min_weight=1, workspace=ws, records=rec, gradients=grd, count=cnt)      # noqa: E731
            run()
            n = int(cnt[0])
            nt = torch_extract(torch, vol, origin, vs, 1)[0].shape[0]
            graph = captured(run)
            tk, tt = [], []
            for _ in range(a.repeats):
                tk.append(timed(graph.replay, a.steps))
                tt.append(timed(lambda: torch_extract(torch, vol, origin, vs, 1), a.torch_steps))
            uk, ut = statistics.median(tk), statistics.median(tt)
            say(f"extract   {N}^3 {scene:5s}: {n} points (torch: {nt}), capacity {cap}")
            say(f"    K24                {spread(tk)}   {N ** 3 * 16 / uk / 1e6:6.3f} TB/s of volume read = {N ** 3 * 16 / uk / 1e6 / HBM_COPY_TBS * 100:5.1f} % "
                f"of the copy rate" + (f"   {uk / forward_us * 100:.2f} % of an S forward" if forward_us else ""))
            say(f"    torch composition  {spread(tt)}   {ut / uk:6.1f}x K24")
            del graph, vol, ref, rec, grd
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
