"""numpy restatement of the VQ-code path (tests only): the corpus reader of preprocess/codes.py,
the padded batch of datasets/codes/dataset.py at r-step ``done`` flags, and argmax."""
import os

import numpy as np


def read_corpus(in_dir, version=0, speaker_info="speaker-info.txt"):
    """``[(key, speaker_id, text, indices)]`` in record order; tab-less first lines left out."""
    speakers = []
    with open(os.path.join(in_dir, speaker_info), encoding="utf8") as f:
        for line in f.readlines()[1:]:
            si = line.split()
            if si and si[0] != "315":
                speakers.append(int(si[0]))
    out = []
    for spk in speakers:
        for name in sorted(os.listdir(in_dir)):
            if not (name.startswith(f"p{spk}") and name.endswith(".txt")):
                continue
            with open(os.path.join(in_dir, name), encoding="utf8") as f:
                parts = f.readline().rstrip("\n").split("\t")
            if len(parts) != 2:
                continue
            codes = [int(c) for c in parts[1].split(" ") if c != ""]
            if version >= 1:
                codes = codes[version - 1::2]
            out.append((name[:-len(".txt")], spk, parts[0], np.array(codes, np.int32)))
    return out


def one_hot(index, C):
    out = np.zeros((len(index), C), np.float32)
    out[np.arange(len(index)), index] = 1.0
    return out


def batch(seqs, C, T_pad, r=1):
    """codes [B, T_pad, C], done [B, T_pad / r], the two masks [B, T_pad], target_length [B]."""
    B = len(seqs)
    codes = np.zeros((B, T_pad, C), np.float32)
    done = np.zeros((B, T_pad // r), np.float32)
    cmask = np.zeros((B, T_pad), np.float32)
    bmask = np.zeros((B, T_pad), np.float32)
    tl = np.zeros(B, np.int64)
    for b, s in enumerate(seqs):
        n = len(s)
        codes[b, :n] = one_hot(np.asarray(s), C)
        if n // r - 1 >= 0:
            done[b, n // r - 1] = 1.0
        cmask[b, :n] = 1.0
        bmask[b, :n] = 1.0
        tl[b] = n
    return codes, done, cmask, bmask, tl


def argmax(x):
    return np.argmax(x, axis=-1).astype(np.int32)
