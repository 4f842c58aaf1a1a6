"""python -m facl_amd.generate_3dv --depth_root D --out_root O: the 3DV dataset from depth frames, on the GPU.

The counterpart of the reference's generate_data/generate_NTU.py `main()` (:77-264).  Clips are found as `:94-118` finds
them, `D/<setup>/nturgb+d_depth_masked/<clip>/*.png` (read through PIL), or as `D/<clip>.npy` holding uint16 (F, H, W).  The
three "resolutions" repeat the clip loop with the same voxel size (:82-92); their folders differ in the random draws only.
Output goes where facl_amd/dataset.py reads: `O/reslution/Resolution{60,30,10}/{raw,others,app}/` (the reference's script
writes `resolution`, its reader reads `reslution`), and with --extract_raw 1 the Resolution60 motion clouds also to `O/raw/`,
the folder the extraction entries list.
"""
import argparse
import os
import queue
import random
import threading

import numpy as np

from . import gen3dv

SUBDIR = 'nturgb+d_depth_masked'            # generate_NTU.py:96
KINDS = (('raw', '.npy'), ('others', '_key.npy'), ('app', '_app.npy'))      # :86-88, :108-110


def find_clips(depth_root):
    """[(clip name, folder of PNGs or path of an .npy)] in the reference's order: sorted setups, sorted clips (:94-103);
    .npy clips of the root itself come first, sorted."""
    if not os.path.isdir(depth_root):
        raise FileNotFoundError("--depth_root %s does not exist" % depth_root)
    clips = [(f[:-4], os.path.join(depth_root, f)) for f in sorted(os.listdir(depth_root)) if f.endswith('.npy')]
    for setup in sorted(os.listdir(depth_root)):
        video = os.path.join(depth_root, setup, SUBDIR)
        if os.path.isdir(video):
            clips += [(c, os.path.join(video, c)) for c in sorted(os.listdir(video))]
    return clips


def load_clip(name, path):
    """uint16 (F, H, W): every frame of the clip, files in sorted order (:117-118)."""
    if os.path.isfile(path):
        a = np.load(path)
        if a.ndim != 3 or a.dtype != np.uint16:
            raise ValueError("clip %s: %s must hold a uint16 (frames, H, W) array, got %s %s" % (name, path, a.dtype, a.shape))
        return a
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("reading depth PNGs needs Pillow (PIL), which does not import here; convert the clips to "
                           "<clip>.npy files holding uint16 (frames, H, W) arrays instead") from e
    files = sorted(os.listdir(path))
    if not files:
        raise ValueError("clip %s: %s holds no frame" % (name, path))
    frames = [np.asarray(Image.open(os.path.join(path, f))) for f in files]
    for f, a in zip(files, frames):
        if a.ndim != 2 or a.shape != frames[0].shape or a.dtype.kind not in 'ui' or a.dtype.itemsize > 4:
            raise ValueError("clip %s: %s is not a single-channel integer depth image of the clip's size" % (name, f))
    return np.stack(frames).astype(np.uint16)


def out_paths(out_root, resolution, name):
    r = os.path.join(out_root, 'reslution', 'Resolution%d' % resolution)
    return [os.path.join(r, sub, name + suffix) for sub, suffix in KINDS]


def write_atomic(path, a):
    """np.save to a temporary name in the same folder, then rename: a reader never sees a partial file."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + '.tmp%d' % os.getpid()
    with open(tmp, 'wb') as f:
        np.save(f, a)
    os.replace(tmp, path)


def _batches(todo, n):
    return [todo[i:i + n] for i in range(0, len(todo), n)]


def _prefetched(batches):
    """Decode batch i+1 on a producer thread while batch i is on the device (the pattern of dataset.DiskBatches)."""
    q = queue.Queue(maxsize=1)
    stop = threading.Event()

    def producer():
        try:
            for batch in batches:
                item = (batch, [load_clip(n, p) for n, p in batch])
                while not stop.is_set():
                    try:
                        q.put(item, timeout=0.1)
                        break
                    except queue.Full:
                        pass
                if stop.is_set():
                    return
            q.put(None)
        except BaseException as e:                        # handed to the consumer, raised there
            q.put(e)

    th = threading.Thread(target=producer, name="facl-gen3dv-decode", daemon=True)
    th.start()
    try:
        while True:
            item = q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item
    finally:
        stop.set()
        while th.is_alive():
            try:
                q.get_nowait()
            except queue.Empty:
                pass
            th.join(timeout=0.05)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--depth_root', required=True)
    p.add_argument('--out_root', required=True)
    p.add_argument('--resolutions', default='60,30,10', help='folder numbers, in the order the reference loops (:82)')
    p.add_argument('--rng', default='numpy', choices=('numpy', 'philox'))
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--batch_clips', type=int, default=8)
    p.add_argument('--voxel_size', type=float, default=30)
    p.add_argument('--extract_raw', type=int, default=0)
    p.add_argument('--overwrite', type=int, default=0)
    p.add_argument('--device', default='cuda')
    return p


def main(argv=None):
    opt = build_parser().parse_args(argv)
    resolutions = [int(r) for r in opt.resolutions.split(',')]
    clips = find_clips(opt.depth_root)
    if not clips:
        raise FileNotFoundError("no clip under %s (expected <setup>/%s/<clip>/*.png or <clip>.npy)" % (opt.depth_root, SUBDIR))
    # one stream pair for the whole run, consumed resolution by resolution, clip by clip, as the reference's main() does
    rng, py = np.random.RandomState(opt.seed & 0xFFFFFFFF), random.Random(opt.seed)
    written = 0
    for ri, res in enumerate(resolutions):
        todo = clips
        if not opt.overwrite:
            todo = [(n, p) for n, p in clips if not all(os.path.exists(q) for q in out_paths(opt.out_root, res, n))]
        for batch, frames in _prefetched(_batches(todo, max(1, opt.batch_clips))):
            names = [n for n, _ in batch]
            outs = gen3dv.generate_clips(frames, names, rng=rng, py_random=py, mode=opt.rng, seed=opt.seed, resolution=ri,
                                         device=opt.device, voxel_size=opt.voxel_size)
            for n, arrays in zip(names, outs):
                for path, a in zip(out_paths(opt.out_root, res, n), arrays):
                    write_atomic(path, a)
                if opt.extract_raw and res == 60:
                    write_atomic(os.path.join(opt.out_root, 'raw', n + '.npy'), arrays[0])
                written += 1
    print("generate_3dv: %d clips x %d resolutions under %s, %d written" % (len(clips), len(resolutions), opt.out_root, written))
    return written


if __name__ == '__main__':
    main()
