"""The contract of include/wordpiece_amd_seen.h as plain Python: the 64-bit row key in Python integers and the set as a
Python set with the state and first rule.  Independent of the library."""
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
CHUNK = 256


def mix64(h):
    h ^= h >> 33
    h = h * 0xFF51AFD7ED558CCD & M64
    h ^= h >> 33
    h = h * 0xC4CEB9FE1A85EC53 & M64
    return h ^ h >> 33


S0 = mix64(G)


def key(row):
    """K(row) of the header for the bytes of a row; a key that comes out 0 is 1"""
    k = mix64(S0 ^ (len(row) | 1 << 40))
    for c in range(0, len(row), CHUNK):
        chunk = row[c:c + CHUNK]
        words = [int.from_bytes(chunk[i:i + 4], "little") for i in range(0, len(chunk), 4)]
        h = mix64(((S0 ^ (c // CHUNK + 1)) + 0x632BE59BD9B4E019) & M64)
        for i in range(0, len(words) - 1, 2):
            h = (mix64(h ^ (words[i] | words[i + 1] << 32)) + G) & M64
        x = (words[-1] if len(words) % 2 else 0) | len(chunk) << 32
        k = (k + mix64(h ^ x)) & M64
    return k or 1


class Seen:
    """the set of a handle"""

    def __init__(self):
        self.keys = set()
        self.stats = None

    def add_keys(self, keys, insert=True):
        """-> (state, first) per key, by the rule of the header; the new keys go into the set unless insert is False"""
        keys = [k or 1 for k in keys]
        smallest, state, first = {}, [], []
        for i, k in enumerate(keys):
            first.append(smallest.setdefault(k, i))
            state.append(2 if k in self.keys else 0 if first[i] == i else 1)
        if insert:
            self.keys.update(keys)
        self.stats = dict(n_rows=len(keys), n_new=state.count(0), n_repeat_batch=state.count(1), n_seen_before=state.count(2), n_keys=len(self.keys))
        return state, first

    def add_rows(self, rows, insert=True):
        """-> {"keys", "state", "first", "kept", "data", "row_off"} for the rows (bytes each) of a batch"""
        keys = [key(r) for r in rows]
        state, first = self.add_keys(keys, insert)
        kept = [i for i, s in enumerate(state) if s == 0]
        off = [0]
        for i in kept:
            off.append(off[-1] + len(rows[i]))
        return dict(keys=keys, state=state, first=first, kept=kept, data=b"".join(rows[i] for i in kept), row_off=off)

    def export(self):
        return sorted(self.keys)
