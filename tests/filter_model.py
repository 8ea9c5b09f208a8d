"""The item filter on the host: test infrastructure, nothing of it comes from the code under test.  The filtered
calls are the unfiltered ones with one more eligibility rule, so this file is tests/chain_model.py's scores and
tests/sample_model.py's keys and log-sum-exp with a mask applied before the selection — it imports those models and
adds only the mask — and the ten-line numpy restatement of revisit-bpr_amd/csrc/bpr_item_filter.h (pack, eligibility,
empty tiles, the next non-empty tile) that the CPU test holds the header to."""
import numpy as np

import sample_model as sm
from chain_model import F, chain_scores, select_rows

TILE, TILE_WORDS = 128, 4


# ---- bpr_item_filter.h, restated --------------------------------------------------------------------------------------
def n_words(I):
    return TILE_WORDS * -(-I // TILE)


def pack(mask):
    """uint32 words of a bool [I] mask: bit i & 31 of word i >> 5; whole tiles; the tail zero"""
    bits = np.zeros(32 * n_words(len(mask)), np.uint64)
    bits[:len(mask)] = mask
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def eligible_items(words, I):
    """bool [I]: what the kernels read out of `words` — item 0 and bits at or past I are nobody's"""
    bits = ((np.asarray(words, np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1).astype(bool)
    ok = bits[:I].copy()
    ok[0] = False
    return ok


def empty_tiles(words, I):
    """bool [ceil(I / 128)]: the tile holds no eligible item"""
    ok = np.zeros(TILE * -(-I // TILE), bool)
    ok[:I] = eligible_items(words, I)
    return ~ok.reshape(-1, TILE).any(axis=1)


def next_tile(words, I, t, t1):
    """the first non-empty tile of [t, t1), or t1"""
    live = np.flatnonzero(~empty_tiles(words, I)[t:t1])
    return t + int(live[0]) if len(live) else t1


# ---- the filtered calls -----------------------------------------------------------------------------------------------
def eligible(words, I, users, indptr, indices):
    """[n, I] bool: sample_model's eligibility (item 0 and the seen row out) and the filter"""
    return sm.eligible(I, users, indptr, indices) & eligible_items(words, I)[None, :]


def topk_rows(P, Q, bias, users, k, words, indptr=None, indices=None):
    """what bpr_topk_rows_filtered / bpr_retrieve_rows_filtered return: (items [n, k] int32, scores [n, k])"""
    users = np.asarray(users)
    S = chain_scores(P[users], Q, bias)
    return select_rows(S, eligible(words, Q.shape[0], users, indptr, indices), k)


def sample_rows(P, Q, bias, users, k, words, indptr=None, indices=None, temperature=1.0, seed=0, draw_ids=None):
    """what bpr_sample_rows_filtered returns: (items, scores, keys [n, k], log_z float64 [n]).  The keys are
    sample_model's — an item's noise does not depend on the filter — and the selection and log_z64 see the mask."""
    users = np.asarray(users)
    I = Q.shape[0]
    draw_ids = users if draw_ids is None else draw_ids
    S = chain_scores(P[users], Q, bias)
    inv_t = sm.inv_temperature(temperature)
    K = sm.keys(S, inv_t, draw_ids, np.arange(I), seed)
    ok = eligible(words, I, users, indptr, indices)
    items, kk = select_rows(K, ok, k)
    sc = np.full(items.shape, -np.inf, F)
    rows = np.nonzero(items >= 0)
    sc[rows] = S[rows[0], items[rows]]
    return items, sc, kk, sm.log_z64(S, ok, inv_t)
