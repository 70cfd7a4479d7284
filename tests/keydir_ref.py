"""A plain model of the key directory (include/fdx.h, f-9): a dict from raw key to dense id
with a capacity, the two modes, the reserved key and the four counters.  The GPU tests compare
fdx_keydir_* against it; tests/test_keydir_ref.py ties it to pandas.factorize."""
import numpy as np

RESERVED = -2 ** 63  # INT64_MIN: the table's empty pattern


class KeyDirModel:
    def __init__(self, capacity: int):
        self.capacity = int(capacity)
        self.reset()

    def reset(self):
        self.ids = {}       # key -> id
        self.key_of = []    # id -> key
        self.refused_full = self.refused_reserved = self.misses = 0

    def map(self, keys, insert=True) -> np.ndarray:
        """Row order IS the numbering order: a new key gets len(key_of) at its first row."""
        out = np.empty(len(keys), np.int32)
        for r, k in enumerate(int(k) for k in keys):
            if k == RESERVED:
                out[r] = -1
                self.refused_reserved += 1
            elif k in self.ids:
                out[r] = self.ids[k]
            elif not insert:
                out[r] = -1
                self.misses += 1
            elif len(self.key_of) < self.capacity:
                out[r] = self.ids[k] = len(self.key_of)
                self.key_of.append(k)
            else:  # full: refused, and not remembered
                out[r] = -1
                self.refused_full += 1
        return out

    def counts(self) -> dict:
        return {"held": len(self.key_of), "refused_full": self.refused_full,
                "refused_reserved": self.refused_reserved, "misses": self.misses}

    def keys(self) -> np.ndarray:
        return np.array(self.key_of, np.int64)

    def load(self, keys):
        keys = [int(k) for k in keys]
        if self.key_of or len(keys) > self.capacity or len(set(keys)) != len(keys) or RESERVED in keys:
            raise ValueError("load refused")
        self.key_of = keys
        self.ids = {k: i for i, k in enumerate(keys)}

    def resized(self, capacity):
        m = KeyDirModel(capacity)
        m.load(self.key_of)
        return m

