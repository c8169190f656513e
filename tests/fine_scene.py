"""Small raw scenes for the fine stage's feed (helper of tests/test_fine_feed_host.py and tests/test_gpu_fine_feed.py, not a test):
cells and poses in the package's data model whose descriptions carry what Kitti360FineDataset reads - is_matched, object_id,
object_instance_id and the four offset fields.  The repository's toy scenes cannot serve: their poses match one object twice, which
the reference's dataset refuses."""
import numpy as np

DIRS = ["north", "south", "east", "west", "on-top"]


def make_fine_scene(n_cells, n_poses, seed, pad_size, num_mentioned=6, scene_name="toy1", lo_pts=10, hi_pts=40):
    """(cells, poses).  Cell i has pad_size + 3 objects (the cut) for i % 4 == 0, exactly pad_size for i % 4 == 1, else 2 ..
    pad_size - 1 (padding); object ids are not their positions (7 * position + 3) and the cell order is not the id order.  Pose q lies
    in cell q % n_cells; of its num_mentioned descriptions k are matched, to k DISTINCT objects of the cell drawn anywhere in it (so
    a matched object can sit behind the cut in cell order) at random hint positions: k = 0 and k = the most the pose allows,
    min(num_mentioned, pad_size, objects of the cell), come up in turn, the rest are drawn in between.  An unmatched description
    names an object id the cell does not hold."""
    from text2pos_amd import data as D, synthetic as S
    rng = np.random.default_rng(seed)
    cells, poses = [], []
    for i in range(n_cells):
        n_obj = pad_size + 3 if i % 4 == 0 else pad_size if i % 4 == 1 else int(rng.integers(2, max(3, pad_size)))
        objs = []
        for j in rng.permutation(n_obj):
            n = int(rng.integers(lo_pts, hi_pts))
            objs.append(D.Object3d(7 * int(j) + 3, 1000 * i + int(j), rng.uniform(-0.3, 1.4, (n, 3)), np.clip(rng.random((n, 3)), 0, 1),
                                   S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 4), 30.0 * (i // 4)
        cells.append(D.Cell(i, scene_name, objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(n_poses):
        c = cells[q % n_cells]
        most = min(num_mentioned, pad_size, len(c.objects))
        turn = (q + q // n_cells) % 4
        k = 0 if turn == 0 else most if turn == 1 else int(rng.integers(1, most + 1))
        picked = [c.objects[int(j)] for j in rng.permutation(len(c.objects))[:k]]
        where = sorted(rng.permutation(num_mentioned)[:k].tolist())
        descs = []
        for h in range(num_mentioned):
            if h in where:
                o = picked[where.index(h)]
                d = D.DescriptionBestCell(DIRS[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                d.object_instance_id = o.instance_id
            else:
                d = D.DescriptionBestCell(DIRS[int(rng.integers(0, 5))], S.COLOR_NAMES[int(rng.integers(0, 8))],
                                          S.LABELS[int(rng.integers(0, len(S.LABELS)))], 9000 + h, False)
                d.object_instance_id = -1
            for name in ("offset_center", "offset_closest", "best_offset_center", "best_offset_closest"):
                setattr(d, name, rng.uniform(-0.5, 0.5, 2))
            descs.append(d)
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, scene_name, descs))
    return cells, poses
