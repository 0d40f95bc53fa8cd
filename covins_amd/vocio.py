"""Reads and writes DBoW2's text vocabulary (TemplatedVocabulary::loadFromTextFile / saveToTextFile, TemplatedVocabulary.h:1338-1460,
descriptors as FORB::fromString / toString write them) into the flat form of covgpu_bow_vocab_t (include/covgpu.h).

The file's first line is `k L scoring weighting`; every further line is one node: `parent is_leaf d0 ... d31 weight`. Node 0 is the root
and has no line; node ids are line order, a node's children are in line order, word ids are leaf order.

Flat form, a dict: k, L, scoring, weighting (ints), parent [N] (parent[0] = -1), child_ptr [N+1], child [N-1], desc [N,32] uint8 (the
root's row is zero), word_id [N] (-1 for an inner node), weight [N] float64 (0 for the root), num_words.

Deliberate divergence: the reference's loader loops `while(!f.eof())`, so a trailing empty line becomes a phantom child of the root
with uninitialised fields. read_text skips blank lines."""
from __future__ import annotations

import numpy as np

L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


def from_nodes(k, L, scoring, weighting, parent, is_leaf, desc, weight):
    """Flat form from per-line arrays (one entry per node below the root, in line order)."""
    parent = np.concatenate([[-1], np.asarray(parent, np.int64)]).astype(np.int32)
    N = len(parent)
    if np.any(parent[1:] < 0) or np.any(parent[1:] >= np.arange(1, N)):
        raise ValueError("a node's parent must come before it")
    leaf = np.concatenate([[False], np.asarray(is_leaf, bool)])
    desc = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(desc, np.uint8).reshape(-1, 32)])
    weight = np.concatenate([[0.0], np.asarray(weight, np.float64)])
    order = np.argsort(parent[1:], kind="stable") + 1          # children grouped by parent, line order within
    child_ptr = np.zeros(N + 1, np.int32)
    child_ptr[1:] = np.cumsum(np.bincount(parent[1:], minlength=N))
    word_id = np.full(N, -1, np.int32)
    word_id[leaf] = np.arange(int(leaf.sum()), dtype=np.int32)
    return dict(k=int(k), L=int(L), scoring=int(scoring), weighting=int(weighting), parent=parent, child_ptr=child_ptr,
                child=order.astype(np.int32), desc=np.ascontiguousarray(desc), word_id=word_id, weight=weight, num_words=int(leaf.sum()))


def read_text(path):
    with open(path) as f:
        head = f.readline().split()
        if len(head) < 4:
            raise ValueError("not a DBoW2 text vocabulary: the first line must be `k L scoring weighting`")
        k, L, scoring, weighting = (int(x) for x in head[:4])
        parent, is_leaf, desc, weight = [], [], [], []
        for line in f:
            t = line.split()
            if not t:
                continue                                         # see the module doc
            if len(t) != 35:
                raise ValueError(f"node line with {len(t)} fields, expected 35")
            parent.append(int(t[0])); is_leaf.append(int(t[1]) > 0)
            desc.append([int(x) for x in t[2:34]]); weight.append(float(t[34]))
    return from_nodes(k, L, scoring, weighting, parent, is_leaf, np.array(desc, np.uint8).reshape(-1, 32), weight)


def write_text(path, voc, trailing_blank_line=False):
    """Writes the flat form; weights in repr precision, so read_text gives the same doubles back."""
    with open(path, "w") as f:
        f.write(f"{voc['k']} {voc['L']} {voc['scoring']} {voc['weighting']}\n")
        for n in range(1, len(voc["parent"])):
            d = " ".join(str(int(x)) for x in voc["desc"][n])
            f.write(f"{int(voc['parent'][n])} {int(voc['word_id'][n] >= 0)} {d} {float(voc['weight'][n])!r}\n")
        if trailing_blank_line:
            f.write("\n")
