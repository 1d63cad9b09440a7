"""A removal from the image index (hesaff_index_remove, include/hesaff_amd.h) in numpy, over tests/index_ref.py as it is: the
definition of a removal is the build of the images that remain, in their order, and the renumbering."""
import numpy as np

from tests import index_ref


def remap(n, gone):
    """int32 [n]: old image i becomes i - #{removed numbers below i}; -1 for a removed one"""
    keep = np.ones(n, bool)
    keep[np.asarray(gone, np.int64)] = False
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def remaining(items, gone):
    """what is left of a per-image list (words, signatures, paths), in order"""
    gone = set(int(i) for i in gone)
    return [x for i, x in enumerate(items) if i not in gone]


def remove(images, gone, k):
    """the index after hesaff_index_remove: index_ref.build of what stays, and the remap"""
    return index_ref.build(remaining(images, gone), k), remap(len(images), gone)
