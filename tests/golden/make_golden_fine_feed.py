"""Writes tests/golden/fine_feed.npz: what the REFERENCE's load_pose_and_cell (dataloading/kitti360pose/poses.py:32-174) makes of a
small scene, for tests/test_fine_feed_host.py::test_feed_against_the_reference_fixture.

    python tests/golden/make_golden_fine_feed.py [reference root; default: make_golden.py's]

The scene of tests/fine_scene.py::make_fine_scene(6, 14, 31, pad_size=8) is rebuilt with the reference's own classes
(datapreparation.kitti360pose.imports) and pickled as the reference's dataset files are; load_pose_and_cell runs on every pose with an
identity transform, once per regressor_cell x regressor_learn combination.  Only data is stored: the two pickles, and per pose the
object ids in list order (-1 = padding), matches, all_matches, the offsets of the four combinations and offsets_best_center.
The reference is imported under make_golden.py's stand-ins plus one for `numpy.lib.function_base`, a module path this NumPy no
longer has (poses.py imports `flip` from it and never uses it)."""
import os
import pickle
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402

PAD_SIZE, NUM_MENTIONED = 8, 6
SCENE = dict(n_cells=6, n_poses=14, seed=31, pad_size=PAD_SIZE, num_mentioned=NUM_MENTIONED, lo_pts=6, hi_pts=14)
COMBOS = [(c, l) for c in ("pose", "best") for l in ("center", "closest")]


def main(ref_root):
    MG.REF = ref_root
    MG.install_standins()
    shim = types.ModuleType("numpy.lib.function_base")
    shim.flip = np.flip
    sys.modules["numpy.lib.function_base"] = shim
    from easydict import EasyDict
    from dataloading.kitti360pose.poses import load_pose_and_cell
    from datapreparation.kitti360pose import imports as RI
    import text2pos_amd  # noqa: F401
    from fine_scene import make_fine_scene
    cells, poses = make_fine_scene(**SCENE)
    ref_cells = {}
    for i, c in enumerate(cells):
        objs = [RI.Object3d(o.id, o.instance_id, o.xyz, o.rgb, o.label) for o in c.objects]
        ref_cells[c.id] = RI.Cell(i, c.scene_name, objs, c.cell_size, c.bbox_w)
        assert ref_cells[c.id].id == c.id
    ref_poses = []
    for p in poses:
        descs = []
        for d in p.descriptions:
            r = RI.DescriptionBestCell.__new__(RI.DescriptionBestCell)
            r.__dict__.update(d.__dict__)
            descs.append(r)
        ref_poses.append(RI.Pose(p.pose, p.pose_w, p.cell_id, p.scene_name, descs))
    out = dict(cells_pkl=np.frombuffer(pickle.dumps(list(ref_cells.values())), dtype=np.uint8),
               poses_pkl=np.frombuffer(pickle.dumps(ref_poses), dtype=np.uint8), pad_size=np.int64(PAD_SIZE),
               num_mentioned=np.int64(NUM_MENTIONED))
    identity = lambda data: data
    for cell_mode, learn in COMBOS:
        args = EasyDict(pad_size=PAD_SIZE, num_mentioned=NUM_MENTIONED, regressor_cell=cell_mode, regressor_learn=learn)
        offsets = []
        for i, p in enumerate(ref_poses):
            hints = [f"The pose is {d.direction} of a {d.object_color_text} {d.object_label}." for d in p.descriptions]
            item = load_pose_and_cell(p, ref_cells[p.cell_id], hints, PAD_SIZE, identity, args)
            offsets.append(np.asarray(item["offsets"], dtype=np.float64))
            if (cell_mode, learn) == COMBOS[0]:
                out[f"ids_{i}"] = np.array([o.id for o in item["objects"]], dtype=np.int64)
                out[f"matches_{i}"] = np.asarray(item["matches"], dtype=np.int64).reshape(-1, 2)
                out[f"all_matches_{i}"] = np.asarray(item["all_matches"], dtype=np.int64).reshape(-1, 2)
                out[f"best_center_{i}"] = np.asarray(item["offsets_best_center"], dtype=np.float64)
                assert item["hint_descriptions"] == hints and item["texts"] == " ".join(hints)
        out[f"offsets_{cell_mode}_{learn}"] = np.stack(offsets)
    path = os.path.join(HERE, "fine_feed.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.REF)
