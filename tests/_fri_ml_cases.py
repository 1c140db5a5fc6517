"""What the CPU and GPU tests of the multilinear FRI opening family share (tests/test_fri_ml_{points,arity,grouped,batch}_cpu.py and
test_gpu_fri_ml_{points,arity,grouped,batch}.py): the checked host hash, the models' commitments and the library's of the same table, points,
and flat arrays padded or with one bit changed.  The seeds stay with the files: each passes its own."""
import functools
import random

import numpy as np

import _fri_ml_grouped_model as GM
import _fri_pcs_model as PM
import _merkle_model as MM
import _ntt_model as NM


@functools.lru_cache(maxsize=None)
def hasher(zk, grouped=False):
    """the library's host Keccak, checked against the model's (grouped: at the quad leaf's 129 bytes too)"""
    return GM.check_host_keccak(zk) if grouped else MM.check_host_keccak(zk)


def coset_of(field, d, b, with_coset, mul):
    return random.Random(mul * d + b + field).randrange(2, NM.MODULUS[field]) if with_coset else 1


def commitment(field, d, b, coset, seed, hasher, grouped=False):
    """the model's commitment (grouped: with its leaves grouped by 4) of the random table of `seed`"""
    return (GM if grouped else PM).commit(field, NM.random_ints(field, 1 << d, seed), b, coset, hasher)


def points_for(field, d, P, seed, bit_at_1=False):
    """P random points, the first with p - 1 as its last coordinate (bit_at_1: and 0 or 1 as its second)"""
    p, rng = NM.MODULUS[field], random.Random(seed)
    pts = [[rng.randrange(p) for _ in range(d)] for _ in range(P)]
    if bit_at_1:
        pts[0][1] = rng.choice((0, 1))
    pts[0][d - 1] = p - 1
    return pts


def gpu_commitment(zk, cm, log_group=None):
    """the library's commitment of a model commitment's table, with the model's leaf grouping unless one is given"""
    from test_gpu_fri import table_of
    cs = None if cm["coset"] == 1 else zk.from_ints(cm["field"], [cm["coset"]])[0]
    return zk.fri.commit(table_of(zk, cm["field"], cm["coeffs"]), cm["b"], cs, log_group=cm.get("log_group", 0) if log_group is None else log_group)


def padded(fl, room=4096):
    """the flat arrays with room behind them: a verifier told another arity, protocol or k reads other counts"""
    return {n: np.concatenate([v.reshape(-1), np.zeros(4 * v.size + room, v.dtype)]) for n, v in fl.items()}


def tampered(base, name, at, rng):
    fl = {n: v.copy() for n, v in base.items()}
    bits = 8 if fl[name].dtype == np.uint8 else 64
    fl[name][at] ^= fl[name].dtype.type(1 << rng.randrange(bits))
    return fl
