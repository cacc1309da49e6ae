"""The io layout (cantorrl_amd/_layout.py) against offsets written out by hand from its formula:

    [obs f32 N x 13 | reward f32 N | terminated u8 N | truncated u8 N | info fields, each 256-B aligned]

then, in the host-mapped block, the actions f32 N x 2, the terminal obs f32 N x 13 and the u32 flag,
each 256-B aligned.  The shapes are the smallest where an alignment or dtype-width slip shows: one env
and no info; five envs with Monitor's f64 columns (57 N and 8 N are no multiples of 256); 256 envs with
all 27 fields, f8 / i4 / f4 mixed (a field is then 2,048 or 1,024 bytes).  No torch, no GPU.
"""
import numpy as np
import pytest

from cantorrl_amd._layout import IoLayout
from cantorrl_amd._lib import INFO_FIELDS

MONITOR_KEYWORDS = ("per_share_step_pnl", "raw_pnl_deviation_abs", "transaction_costs_total")
ALL = tuple(k for k, _ in INFO_FIELDS)
WIDTH = {"f8": 8, "i4": 4, "f4": 4}
NP = {"f8": np.float64, "i4": np.int32, "f4": np.float32}

# n, keys, by hand: reward, terminated, truncated, info0, total, actions, terminal obs, flag
CASES = [
    # 58 -> 256; no fields; 256 + 8 = 264 -> 512; 512 + 52 = 564 -> 768
    (1, (), 52, 56, 57, 256, 256, 256, 512, 768),
    # 5 * 58 = 290 -> 512; four f64 columns of 40 B, 256 apart: 512 + 4 * 256; + 40 -> 1792; + 260 = 2052 -> 2304
    (5, MONITOR_KEYWORDS + ("reward_step",), 260, 280, 285, 512, 1536, 1536, 1792, 2304),
    # 256 * 58 = 14848 (= 58 * 256); 12 f8 x 2048 + 15 (i4 / f4) x 1024 = 39936; + 2048; + 13312
    (256, ALL, 13312, 14336, 14592, 14848, 54784, 54784, 56832, 70144),
]


def _by_hand(n, keys):
    """{key: (offset, bytes, numpy type)} from the formula: each field starts at the next multiple of 256."""
    typ = dict(INFO_FIELDS)
    o = -(-58 * n // 256) * 256
    out = {}
    for k in keys:
        out[k] = (o, n * WIDTH[typ[k]], NP[typ[k]])
        o = -(-(o + n * WIDTH[typ[k]]) // 256) * 256
    return out, o


@pytest.mark.parametrize("n,keys,reward,term,trunc,info0,total,act,tobs,flag", CASES,
                         ids=["n1_no_info", "n5_monitor", "n256_all_fields"])
def test_layout_offsets_and_views(n, keys, reward, term, trunc, info0, total, act, tobs, flag):
    L = IoLayout(n, keys)
    assert (L.reward, L.terminated, L.truncated, L.info0, L.total) == (reward, term, trunc, info0, total)
    assert (L.actions, L.terminal_obs, L.flag, L.host_total) == (act, tobs, flag, flag + 4)
    hand, end = _by_hand(n, keys)
    assert end == total and list(L.fields) == list(keys)
    spans = [(0, 52 * n), (reward, reward + 4 * n), (term, term + n), (trunc, trunc + n)]
    for k in keys:
        dt, o, b = L.fields[k]
        assert (o, b, dt) == (hand[k][0], hand[k][1], np.dtype(hand[k][2])), k
        assert o % 256 == 0 and o >= info0, k
        spans.append((o, o + b))
    spans += [(act, act + 8 * n), (tobs, tobs + 52 * n), (flag, flag + 4)]
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):   # in buffer order, nothing overlaps
        assert a0 < a1 <= b0, (spans,)
    assert spans[-1][1] == L.host_total and all(s % 256 == 0 for s, _ in spans[-3:])

    # a byte pattern whose value encodes its own offset: u32 word w holds w (so byte o belongs to word o // 4)
    buf = np.arange(L.host_total // 4, dtype=np.uint32).view(np.uint8)
    word = lambda off, count, typ: np.arange(off // 4, off // 4 + count, dtype=np.uint32).view(typ)  # noqa: E731
    obs, rew, done = L.unpack(buf[:L.truncated])
    assert obs.shape == (n, 13) and obs.dtype == np.float32 and obs.tobytes() == word(0, 13 * n, np.float32).tobytes()
    assert rew.shape == (n,) and rew.dtype == np.float32 and rew.tobytes() == word(reward, n, np.float32).tobytes()
    assert done.shape == (n,) and done.dtype == np.bool_ and done.tobytes() == buf[term:term + n].tobytes()
    o2, r2 = L.obs_reward(buf[:L.terminated])
    assert o2.tobytes() == obs.tobytes() and r2.tobytes() == rew.tobytes()
    info = L.split_info(buf[info0:total])
    assert list(info) == list(keys)
    for k in keys:
        o, b, typ = hand[k]
        assert info[k].shape == (n,) and info[k].dtype == typ and info[k].tobytes() == buf[o:o + b].tobytes(), k
        assert np.shares_memory(info[k], buf)   # views, not copies
    # the same bytes through the record dtype
    rec = buf[:total].view(L.record_dtype())
    assert rec.shape == (1,)
    assert rec["obs"][0].tobytes() == obs.tobytes() and rec["reward"][0].tobytes() == rew.tobytes()
    assert rec["terminated"][0].tobytes() == buf[term:term + n].tobytes()
    for k in keys:
        assert rec[k][0].tobytes() == info[k].tobytes(), k
    # and env 0's value of each field through a gather in the field's own width
    for code, typ in NP.items():
        ks = [k for k in keys if dict(INFO_FIELDS)[k] == code]
        got = buf[:total].view(typ)[L.gather_index(ks)]
        assert [g.tobytes() for g in got] == [info[k][:1].tobytes() for k in ks]


def test_record_fields_are_scalars_for_one_env():
    """HedgingEnv reads its one env's record field by field: plain scalars, not [1] columns."""
    rec = np.zeros(1, IoLayout(1, ALL).record_dtype())[0]
    assert rec["obs"].shape == (13,) and rec["reward"].shape == () and rec["current_step"].shape == ()
    assert IoLayout(5, ALL).record_dtype()["cash"].shape == (5,)


def test_unknown_info_key_is_refused():
    with pytest.raises(KeyError, match="no_such_field"):
        IoLayout(2, ("cash", "no_such_field"))
