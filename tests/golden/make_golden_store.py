#!/usr/bin/env python3
"""Generate tests/golden/store.npz by running the REFERENCE's ImageFeaturesH5Reader.__getitem__ (sam/datasets/_image_features_reader.py) on CPU, in both
of its modes (in_memory=True, the cached branch the training uses, and in_memory=False).

Runs ONLY in the build container (the reference never travels to the GPU box).  The reader imports `lmdb` and `h5py`, neither of which is installed:
stub modules of those names go into sys.modules before the import -- h5py is never called; lmdb.open() returns an environment whose transactions serve
pickles from a dict, the way an LMDB of the reference's schema would ({image_id: pickle({"features", "boxes", "image_w", "image_h"}), b"keys": pickle of
the id list}).  Nothing of the reference's program text is stored: the fixture holds data only.

store.npz, per image g (arrays named <name>_<g>):
    boxes_g    float32 [n, 4]   pixel xyxy, as the LMDB item holds them
    size_g     int64 [2]        image_w, image_h
    loc_g      float32 [n, 5]   the reader's image_location WITHOUT its row 0 (the prepended [0, 0, 1, 1, 1]); the reader returns float64 that holds
                                float32 values exactly (its np.concatenate with an integer row), asserted here
    first_g    float64 [5]      the reader's row 0
and `seed`: the feature rows are np.random.RandomState(seed + g).rand(n, 2048).astype(float32) -- the reader passes them through untouched behind its
average row (asserted here), so the tests regenerate them and the fixture does not store them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_store.py
"""
import importlib
import os
import pickle
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import REF  # noqa: E402

SEED = 325


def images():
    """(boxes float32 [n, 4], w, h): n in {0, 1, 2, 7}; sizes whose w * h is not a float32 (4999 x 3001 = 15001999 > 2^24, odd); non-integer pixel
    coordinates; degenerate boxes (zero width, zero height, a point, x2 < x1); a box on the image border; a tiny and a huge image"""
    rng = np.random.RandomState(SEED)

    def rand_boxes(n, w, h):
        a = rng.rand(n, 2) * [w, h] * 0.7
        b = a + rng.rand(n, 2) * [w, h] * 0.3
        return np.concatenate([a, b], 1).astype(np.float32)

    out = [(np.zeros((0, 4), np.float32), 640, 480),
           (np.array([[10.5, 20.25, 300.75, 400.125]], np.float32), 1024, 768),
           (rand_boxes(2, 4999, 3001), 4999, 3001),
           (rand_boxes(7, 4999, 3001), 4999, 3001),
           (rand_boxes(7, 333, 1777), 333, 1777),
           (np.array([[5.0, 5.0, 5.0, 90.0], [5.0, 7.5, 80.0, 7.5], [33.3, 44.4, 33.3, 44.4], [90.0, 10.0, 20.0, 60.0], [0.0, 0.0, 127.0, 97.0],
                      [0.1, 0.2, 0.3, 0.7], [126.99, 96.99, 127.0, 97.0]], np.float32), 127, 97),
           (rand_boxes(2, 7, 3), 7, 3),
           (rand_boxes(7, 16385, 12289), 16385, 12289)]
    assert sorted({b.shape[0] for b, _, _ in out}) == [0, 1, 2, 7]
    assert any(float(np.float32(float(w) * float(h))) != float(w) * float(h) for _, w, h in out)
    return out


def features_of(g, n):
    return np.random.RandomState(SEED + g).rand(n, 2048).astype(np.float32)


def install_stubs(db):
    class Txn:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def get(self, key):
            return db[key]

    class Env:
        def begin(self, write=False):
            return Txn()

    lmdb = types.ModuleType("lmdb")
    lmdb.open = lambda path, **kw: Env()
    sys.modules["lmdb"] = lmdb
    sys.modules["h5py"] = types.ModuleType("h5py")
    for name, path in (("sam", os.path.join(REF, "sam")), ("sam.datasets", os.path.join(REF, "sam", "datasets"))):       # bare packages: their __init__ is not run
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg


def main():
    imgs = images()
    ids = [("img_%d" % g).encode() for g in range(len(imgs))]
    db = {b"keys": pickle.dumps(ids)}
    for g, (boxes, w, h) in enumerate(imgs):
        db[ids[g]] = pickle.dumps({"features": features_of(g, boxes.shape[0]), "boxes": boxes.copy(), "image_w": w, "image_h": h})
    install_stubs(db)
    Reader = importlib.import_module("sam.datasets._image_features_reader").ImageFeaturesH5Reader
    cached, direct = Reader("unused", in_memory=True), Reader("unused", in_memory=False)
    arrays = {"seed": np.array(SEED, np.int64)}
    for g, (boxes, w, h) in enumerate(imgs):
        n = boxes.shape[0]
        feats, num, loc, _ = cached["img_%d" % g]
        again = cached["img_%d" % g]                                  # the second call takes the cached branch
        assert num == n + 1 and loc.shape == (n + 1, 5) and feats.shape == (n + 1, 2048) and again[1] == num and np.array_equal(again[2], loc)
        assert np.array_equal(feats[1:], features_of(g, n))          # the rows pass through untouched
        if n:                                                        # (the uncached branch divides by num_boxes: n = 0 gives it NaN rows and a warning)
            d = direct["img_%d" % g]
            assert d[1] == num and np.array_equal(d[2], loc)
        assert np.array_equal(loc[1:].astype(np.float32).astype(loc.dtype), loc[1:])            # float32 values in a float64 array
        arrays["boxes_%d" % g] = boxes
        arrays["size_%d" % g] = np.array([w, h], np.int64)
        arrays["loc_%d" % g] = loc[1:].astype(np.float32)
        arrays["first_%d" % g] = np.asarray(loc[0], np.float64)
    out = os.path.join(HERE, "store.npz")
    np.savez_compressed(out, **arrays)
    print("%s: %d images, %d bytes" % (out, len(imgs), os.path.getsize(out)))


if __name__ == "__main__":
    main()
