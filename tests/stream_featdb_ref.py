"""numpy restatement of specification FD-2: what one step of a stream set stores in the attached device feature DB.
Written from the specification's sentences, not from csrc/stream_featdb.hip; it does not import the library.  The state is the DB's
array over its whole capacity, the count and (level 11) the DB row every stream owns; step() works on host tables and counts the arms
it takes in `arms`."""
import collections

import numpy as np

WIDTH = {5: 53, 13: 53, 11: 264, 12: 23}
FLAG_CAPACITY, FLAG_DB_FULL = 1, 16


class State:
    def __init__(self, level, capacity, n_streams=0, fill=None):
        self.level, self.width, self.capacity = level, WIDTH[level], int(capacity)
        self.db = np.zeros((self.capacity, self.width)) if fill is None else np.array(fill, np.float64).reshape(self.capacity, self.width)
        self.count = 0
        self.slot = np.full(n_streams, -1, np.int32)
        self.arms = collections.Counter()

    def rows(self):
        return self.db[:self.count]


def _marked(x):
    return not (x == 0)                                  # NaN != 0: marked; -0 == 0: not


def step(st, meta=None, feat=None, utt_off=None, bits=None, flags=0):
    """One step.  Levels 5 / 12 / 13: meta [n][8], feat [n][53] = the step's compacted rows in (stream, callback) order.  Level 11:
    feat [n][264] = the step's utterance rows, utt_off [n_streams + 1], bits [n_streams] (bit 0: START).  flags: the step's flags.
    Returns dict(first_row, n_added, n_replaced, not_fitted, kept, replaced, flags) — flags with FLAG_DB_FULL added where it applies."""
    a = st.arms
    feat = np.asarray(feat, np.float64).reshape(-1, 264 if st.level == 11 else 53)
    out = dict(first_row=st.count, n_added=0, n_replaced=0, not_fitted=0, kept=np.zeros(0, np.int32),
               replaced=np.zeros((0, 2), np.int32) if st.level == 11 else None, flags=int(flags))
    bad = bool(flags & FLAG_CAPACITY)
    if st.level == 11:
        # START forgets the stream's row before the step's results are looked at — in every step, stored or not
        slot = st.slot.copy()
        for i in range(len(slot)):
            if int(bits[i]) & 1:
                a["l11_start_with_row" if slot[i] >= 0 else "l11_start_without_row"] += 1
                slot[i] = -1
        st.slot = slot
        if bad:
            a["capacity_flag"] += 1
            return out
        active = [i for i in range(len(slot)) if int(utt_off[i]) < int(utt_off[i + 1])]
        a["l11_idle_stream"] += len(slot) - len(active)
        fresh = [i for i in active if slot[i] < 0]
        if st.count + len(fresh) > st.capacity:
            a["full_with_replacements" if len(fresh) < len(active) else "full"] += 1
            out["not_fitted"] = len(fresh)
            out["flags"] |= FLAG_DB_FULL
            return out
        a["fits_exactly" if fresh and st.count + len(fresh) == st.capacity else "fits"] += 1
        kept, replaced = [], []
        for i in active:
            last = int(utt_off[i + 1]) - 1
            if int(utt_off[i + 1]) - int(utt_off[i]) > 1:
                a["l11_several_results"] += 1
            if slot[i] < 0:
                a["l11_new_row"] += 1
                slot[i] = st.count + len(kept)
                kept.append(last)
            else:
                a["l11_replaced"] += 1
                replaced.append((last, int(slot[i])))
            st.db[slot[i]] = feat[last]
        st.count += len(kept)
        out.update(n_added=len(kept), n_replaced=len(replaced), kept=np.array(kept, np.int32), replaced=np.array(replaced, np.int32).reshape(-1, 2))
        return out
    if bad:
        a["capacity_flag"] += 1
        return out
    if st.level in (5, 13):
        a["all_rows"] += 1
        kept = list(range(len(feat)))
    else:
        kept, marked_from = [], {}
        for r in range(len(feat)):
            key = (int(meta[r][0]), int(meta[r][1]))
            if _marked(feat[r, 23]):
                a["l12_mark_nan" if feat[r, 23] != feat[r, 23] else "l12_mark"] += 1
                if key not in marked_from:
                    a["l12_mark_on_first_row" if r == 0 or (int(meta[r - 1][0]), int(meta[r - 1][1])) != key else "l12_mark_later"] += 1
                marked_from.setdefault(key, r)
            elif np.signbit(feat[r, 23]):
                a["l12_minus_zero"] += 1
            if key in marked_from:
                a["l12_dropped"] += 1
            else:
                kept.append(r)
    if not kept:
        a["nothing_to_store"] += 1
    if st.count + len(kept) > st.capacity:
        a["full"] += 1
        out["not_fitted"] = len(kept)
        out["flags"] |= FLAG_DB_FULL
        return out
    a["fits_exactly" if kept and st.count + len(kept) == st.capacity else "fits"] += 1
    if kept:
        st.db[st.count:st.count + len(kept)] = feat[kept, :st.width]
    st.count += len(kept)
    out.update(n_added=len(kept), kept=np.array(kept, np.int32))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
