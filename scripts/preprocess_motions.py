#!/usr/bin/env python3
"""Dataset preprocessing on the GPU: the reference's ``compute_preprocessing_data`` pass of ``create_dataset.py``
(``terrain_util.compute_hf_extra_vals`` on every file), for every file in ONE batched run.

    python scripts/preprocess_motions.py data/motion_terrains [more folders, .pkl files or dataset YAMLs] \\
        [--output_dir DIR] [--override_old_hf_mask_inds] [--z_buf 3.0] [--jump_buf 0.8]

Writes ``misc_data["hf_mask_inds"]`` (a list of int64 [K, 2] arrays, one per frame) and ``terrain_data.hf_maxmin``; the motion
payload is kept byte for byte and every other terrain / misc field unchanged.  A file that already carries mask inds is kept as it is
unless ``--override_old_hf_mask_inds``; one whose misc data holds ``hf_mask_inds: None`` (what the recorder writes) has none and is
preprocessed.  Files are replaced atomically (a temporary file in the same folder, then a rename).  A file whose misc payload the data-only decoder cannot read (it would be dropped on
rewriting) is refused: the script lists such files and exits non-zero before writing anything.  ``--output_dir`` writes the results
(and unchanged copies of the kept files) there instead of rewriting in place.
"""
import argparse
import os
import pickle
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import ms_file  # noqa: E402

HF_MASK_INDS_KEY = "hf_mask_inds"   # file_io_helper.HF_MASK_INDS_KEY


def gather_files(inputs):
    """Folders (every .pkl below, sorted), dataset YAMLs (their ``motions`` entries) and single .pkl files, in order, without repeats."""
    from parc_amd.motion_lib import fetch_motion_files
    out = []
    for p in inputs:
        if os.path.isdir(p):
            for root, _, names in sorted(os.walk(p)):
                out += [os.path.join(root, n) for n in sorted(names) if n.endswith(".pkl")]
        elif p.endswith(".yaml"):
            out += fetch_motion_files(p)[0]
        else:
            out.append(p)
    seen, files = set(), []
    for f in out:
        r = os.path.realpath(f)
        if r not in seen:
            seen.add(r)
            files.append(f)
    return files


def read_container(path):
    """(container dict of payload bytes, decoded terrain dict, decoded misc dict or None, misc dropped?)."""
    with open(path, "rb") as f:
        container = ms_file.loads_data_only(f.read())
    if not isinstance(container, dict) or container.get(ms_file.TERRAIN_DATA_KEY) is None or \
            container.get(ms_file.MOTION_DATA_KEY) is None:
        raise ValueError(f"{path}: not a motion-terrain file with motion and terrain data")
    terrain = ms_file.loads_data_only(container[ms_file.TERRAIN_DATA_KEY])
    misc, dropped = None, False
    if container.get(ms_file.MISC_DATA_KEY) is not None:
        try:
            misc = ms_file.loads_data_only(container[ms_file.MISC_DATA_KEY])
        except ms_file.UnsafePickleError:
            dropped = True
    return container, terrain, misc, dropped


def has_mask_inds(misc):
    """The reference stores the key only with a value (file_io_helper.py:137); the recorder's ``None`` means no mask inds."""
    return isinstance(misc, dict) and misc.get(HF_MASK_INDS_KEY) is not None


def write_container(path, container, terrain, misc):
    """Replaces ``path`` atomically: an interrupted write leaves the old file intact."""
    out = dict(container)
    out[ms_file.TERRAIN_DATA_KEY] = pickle.dumps(terrain)
    out[ms_file.MISC_DATA_KEY] = pickle.dumps(misc)
    fd, tmp = tempfile.mkstemp(prefix=".preprocess_", suffix=".pkl", dir=os.path.dirname(os.path.abspath(path)))
    try:
        with os.fdopen(fd, "wb") as f:
            pickle.dump(out, f)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def run(files, output_dir=None, override=False, z_buf=3.0, jump_buf=0.8, analyzer=None, char_file=None, device="cuda:0", log=print):
    """Returns (written, kept) paths.  ``analyzer``: anything with ``analyze(clips, z_buf=, jump_buf=)`` (default: the GPU
    ``MotionTerrainAnalyzer``)."""
    from parc_amd.motion_opt import clip_from_ms
    entries, refused = [], []
    for f in files:
        container, terrain, misc, dropped = read_container(f)
        if dropped:
            refused.append(f)
        entries.append((f, container, terrain, misc))
    if refused:
        raise SystemExit("refusing to rewrite files whose misc data the data-only decoder cannot read (it would be lost):\n  " +
                         "\n  ".join(refused))
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        names = [os.path.basename(f) for f in files]
        if len(set(names)) != len(names):
            raise SystemExit("--output_dir: input files share a file name")
    redo = [override or not has_mask_inds(e[3]) for e in entries]
    todo = [e for e, r in zip(entries, redo) if r]
    kept = [e[0] for e, r in zip(entries, redo) if not r]
    dest = (lambda f: os.path.join(output_dir, os.path.basename(f))) if output_dir else (lambda f: f)
    written = []
    if todo:
        if analyzer is None:
            from parc_amd.motion_terrain import MotionTerrainAnalyzer
            analyzer = MotionTerrainAnalyzer(char_file or os.path.join(REPO, "data/assets/humanoid.xml"), device)
        res = analyzer.analyze([clip_from_ms(e[0]) for e in todo], z_buf=z_buf, jump_buf=jump_buf)
        for (f, container, terrain, misc), r in zip(todo, res):
            terrain = dict(terrain)
            terrain["hf_maxmin"] = np.ascontiguousarray(r["hf_maxmin"], np.float32)
            misc = dict(misc or {})
            misc[HF_MASK_INDS_KEY] = [np.ascontiguousarray(a, np.int64) for a in r["hf_mask_inds"]]
            write_container(dest(f), container, terrain, misc)
            written.append(dest(f))
    for f in kept:
        if output_dir:
            shutil.copyfile(f, dest(f))
    log(f"preprocessed {len(written)} files, kept {len(kept)} that already had {HF_MASK_INDS_KEY}")
    return written, [dest(f) for f in kept]


def main(argv=None, analyzer=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("inputs", nargs="+", help="folders, .pkl files or dataset YAMLs")
    ap.add_argument("--output_dir", default=None)
    ap.add_argument("--override_old_hf_mask_inds", action="store_true")
    ap.add_argument("--z_buf", type=float, default=3.0)
    ap.add_argument("--jump_buf", type=float, default=0.8)
    ap.add_argument("--char_file", default=os.path.join(REPO, "data/assets/humanoid.xml"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    return run(gather_files(a.inputs), a.output_dir, a.override_old_hf_mask_inds, a.z_buf, a.jump_buf, analyzer, a.char_file, a.device)


if __name__ == "__main__":
    main()
