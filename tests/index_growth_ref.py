"""The growing, durable index of include/hesaff_amd.h (hesaff_index_add, hesaff_index_save / hesaff_index_load) in numpy, over
tests/index_ref.py and tests/embedding_ref.py as they are: the definition of an add is the build of the old images followed by the
new ones, the lists of an index as per-word sorted multisets, and the index file written and taken apart byte by byte."""
import numpy as np

from tests import index_ref

MAGIC = b"HESAFFI1"
HEAD = 40


def add(old_images, new_images, k):
    """the index after hesaff_index_add: index_ref.build over the concatenated collection"""
    return index_ref.build(list(old_images) + list(new_images), k)


def postings(index, k):
    """per word the sorted list of (image, tf) of index_ref.build's result"""
    lists = [[] for _ in range(k)]
    for i, (words, counts) in enumerate(index[0]):
        for w, c in zip(words.tolist(), counts.tolist()):
            lists[w].append((i, c))
    return lists   # (images ascend: sorted)


def key_lists(images, sigs, k):
    """per word the sorted list of (image, signature) of an embedded index"""
    lists = [[] for _ in range(k)]
    for i, (words, g) in enumerate(zip(images, sigs)):
        for w, s in zip(np.asarray(words).tolist(), np.asarray(g, np.uint64).tolist()):
            lists[w].append((i, s))
    return [sorted(l) for l in lists]


def split_lists(offsets, first, second):
    """the arrays of index_postings() / index_embedded() -> per word the sorted list of pairs"""
    o = np.asarray(offsets, np.int64)
    a, b = np.asarray(first).tolist(), np.asarray(second).tolist()
    return [sorted(zip(a[o[w]:o[w + 1]], b[o[w]:o[w + 1]])) for w in range(len(o) - 1)]


def file_arrays(images, k, sigs=None):
    """the arrays of an index file of this collection, lists in ascending order: (n_images, n_keys, df, postings [n, 2], key_count,
    key_image, key_sig), the last three None without signatures"""
    index = index_ref.build(images, k)
    flat = [p for l in postings(index, k) for p in l]
    post = np.array(flat, np.uint32).reshape(-1, 2)
    n_keys = sum(len(w) for w in images)
    if sigs is None:
        return len(images), n_keys, index[1].copy(), post, None, None, None
    kl = key_lists(images, sigs, k)
    flat = [p for l in kl for p in l]
    return (len(images), n_keys, index[1].copy(), post, np.array([len(l) for l in kl], np.uint32), np.array([p[0] for p in flat], np.uint32),
            np.array([p[1] for p in flat], np.uint64))


def _pad8(b):
    return b + b"\0" * (-len(b) % 8)


def file_bytes(n_images, n_keys, df, post, key_count=None, key_image=None, key_sig=None, flags=None, reserved=0, k=None, n_postings=None):
    """the file of the format, field by field; flags, reserved, k and n_postings may be forced to make a file that is not one"""
    embedded = key_count is not None
    head = MAGIC + np.array([int(embedded) if flags is None else flags, len(df) if k is None else k, n_images, reserved], "<u4").tobytes() + \
        np.array([n_keys, len(post) if n_postings is None else n_postings], "<u8").tobytes()
    assert len(head) == HEAD
    out = head + _pad8(np.asarray(df, "<u4").tobytes()) + np.asarray(post, "<u4").tobytes()
    if embedded:
        out += _pad8(np.asarray(key_count, "<u4").tobytes()) + _pad8(np.asarray(key_image, "<u4").tobytes()) + np.asarray(key_sig, "<u8").tobytes()
    return out


def layout(k, n_keys, n_postings, embedded):
    """byte offsets (df, postings, key_count, key_image, key_sig, size) of a file's arrays"""
    df = HEAD
    post = df + (4 * k + 7) // 8 * 8
    kc = post + 8 * n_postings
    if not embedded:
        return df, post, kc, kc, kc, kc
    ki = kc + (4 * k + 7) // 8 * 8
    ks = ki + (4 * n_keys + 7) // 8 * 8
    return df, post, kc, ki, ks, ks + 8 * n_keys
