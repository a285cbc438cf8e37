"""The integer twin of crn_hops_device and the Python of crn_hop_forecast, written from the definition in include/crn_sense.h (plain numpy
and Python, one epoch after the other: the sequential rule, nothing of the kernels' chunks, parts and joins):

  states   C = n_channels; the augmented word of an epoch is a = w & ((1 << C) - 1), and 1 << 63 when that is 0
  record   int64 n_epochs, int32 n_channels, n_lags, lag[8], reserved[4]; uint64 hist[64] (bit k of hist[c]: bit c of the augmented word
           of epoch n_epochs - 1 - k); int32 hop[64][64]; per lag int32 from[64], to[64], pair[64][64]
  rule     per epoch, T = n_epochs before it, cur = its augmented word:
               for each lag m with T >= lag[m]: prev = the word of epoch T - lag[m]; from[m][i] += 1 for i in prev, to[m][j] += 1 for j
                   in cur, pair[m][i][j] += 1 for every such i, j
               if T >= 1: prev = the word of epoch T - 1; hop[i][j] += 1 for i in prev & ~cur and j in cur & ~prev
               cur is shifted into hist; n_epochs += 1;  every int32 count saturates at 2^31 - 1
  carry    taken as empty when first, when n_epochs <= 0, or when n_channels, n_lags or any lag[] differs from the call's; hist is
           masked to k < min(n_epochs, 64) and to the positions c < C and c = 63; a negative count is read as 0

`update` steps the records of a batch (bytes in, bytes out); `forecast` is crn_hop_forecast."""
import numpy as np

SAT = 2 ** 31 - 1
IDLE = 63
M64 = 2 ** 64 - 1


def dtype(n_lags):
    return np.dtype([("n_epochs", "<i8"), ("n_channels", "<i4"), ("n_lags", "<i4"), ("lag", "<i4", (8,)), ("reserved", "<i4", (4,)),
                     ("hist", "<u8", (64,)), ("hop", "<i4", (64, 64)),
                     ("lags", [("from", "<i4", (64,)), ("to", "<i4", (64,)), ("pair", "<i4", (64, 64))], (n_lags,))])


def record_bytes(n_lags):
    return 64 + 512 + 16384 + n_lags * 16896


def augment(w, C):
    a = int(w) & ((1 << C) - 1)
    return a if a else 1 << IDLE


def bits(a):
    """The 64 bits of a word as a 0 / 1 vector of int64."""
    return np.unpackbits(np.array([a], "<u8").view(np.uint8), bitorder="little").astype(np.int64)


class State:
    """One stream's record as Python ints and int64 arrays: what the rule steps."""

    def __init__(self, C, lags):
        self.C, self.lags = C, list(lags)
        self.n_epochs = 0
        self.words = []                       # the augmented words of the last 64 epochs, newest first
        self.hop = np.zeros((64, 64), np.int64)
        self.frm = np.zeros((len(lags), 64), np.int64)
        self.to = np.zeros((len(lags), 64), np.int64)
        self.pair = np.zeros((len(lags), 64, 64), np.int64)

    @classmethod
    def read(cls, rec, C, lags, first):
        """The carried record `rec` (one element of dtype(len(lags))) as the rule reads it."""
        s = cls(C, lags)
        want = list(lags) + [0] * (8 - len(lags))
        if first or int(rec["n_epochs"]) <= 0 or int(rec["n_channels"]) != C or int(rec["n_lags"]) != len(lags) or rec["lag"].tolist() != want:
            return s
        s.n_epochs = int(rec["n_epochs"])
        seen = min(s.n_epochs, 64)
        chans = [c for c in range(64) if c < C or c == IDLE]
        s.words = [sum(((int(rec["hist"][c]) >> k) & 1) << c for c in chans) for k in range(seen)]
        s.hop = np.maximum(rec["hop"].astype(np.int64), 0)
        s.frm = np.maximum(rec["lags"]["from"].astype(np.int64), 0)
        s.to = np.maximum(rec["lags"]["to"].astype(np.int64), 0)
        s.pair = np.maximum(rec["lags"]["pair"].astype(np.int64), 0)
        return s

    def step(self, w):
        T, cur = self.n_epochs, augment(w, self.C)
        cb = bits(cur)
        for m, d in enumerate(self.lags):
            if T >= d:
                pb = bits(self.words[d - 1])
                self.frm[m] = np.minimum(self.frm[m] + pb, SAT)
                self.to[m] = np.minimum(self.to[m] + cb, SAT)
                self.pair[m] = np.minimum(self.pair[m] + np.outer(pb, cb), SAT)
        if T >= 1:
            prev = self.words[0]
            self.hop = np.minimum(self.hop + np.outer(bits(prev & ~cur & M64), bits(cur & ~prev & M64)), SAT)
        self.words = ([cur] + self.words)[:64]
        self.n_epochs = min(T + 1, 2 ** 63 - 1)

    def write(self, rec):
        rec["n_epochs"], rec["n_channels"], rec["n_lags"] = self.n_epochs, self.C, len(self.lags)
        rec["lag"] = self.lags + [0] * (8 - len(self.lags))
        rec["reserved"] = 0
        rec["hist"] = [sum(((w >> c) & 1) << k for k, w in enumerate(self.words)) for c in range(64)]
        rec["hop"] = self.hop
        rec["lags"]["from"], rec["lags"]["to"], rec["lags"]["pair"] = self.frm, self.to, self.pair


def update(records, busy, C, lags, epochs_per_stream, first):
    """records: the bytes (or uint8 array) of the carried records, one per stream, or None with first; busy [E] uint64.  Returns the new
    records as an array of dtype(len(lags)), one per stream."""
    busy = np.asarray(busy, np.uint64)
    n_streams = busy.size // epochs_per_stream if epochs_per_stream else 0
    dt = dtype(len(lags))
    old = np.zeros(n_streams, dt) if records is None else np.frombuffer(bytes(records), dt)[:n_streams]
    new = old.copy()
    if busy.size == 0:
        return new
    for st in range(n_streams):
        s = State.read(old[st], C, lags, first)
        for w in busy[st * epochs_per_stream: (st + 1) * epochs_per_stream].tolist():
            s.step(w)
        s.write(new[st])
    return new


def sequence(words, C, lags):
    """One stream from nothing: the record after the busy words `words`."""
    return update(None, np.array(list(words), np.uint64), C, lags, max(len(words), 1), True)[0] if len(words) else np.zeros(1, dtype(len(lags)))[0]


def forecast(rec, m, word, prior):
    """crn_hop_forecast: p[j] = the largest over the set bits i of the augmented word of (pair[m][i][j] + prior) / (from[m][i] + 2 prior);
    0 / 0 gives 0.5; p[j] = 0 for C <= j < 63."""
    C = int(rec["n_channels"])
    a = augment(word, C)
    p = np.zeros(64)
    for i in range(64):
        if (a >> i) & 1:
            den = max(int(rec["lags"]["from"][m][i]), 0) + 2.0 * prior
            for j in list(range(C)) + [IDLE]:
                q = (max(int(rec["lags"]["pair"][m][i][j]), 0) + prior) / den if den > 0 else 0.5
                p[j] = max(p[j], q)
    return p
