"""The feature DB that stays on the device: the host half of specifications FD-1 and FD-2 (K10 and the stream step's DB
kernels are the device half, capi.FeatDB).
What the reference application does between analysing and learning: src/index.js:35-100 (call_backed -> StoreFeatures) files every
callback's vectors under (db, file, part) — js/featuredb.js is this library's writer of the same format — and training, prediction, the
results table and the KNN learner then read that DB.  Here the FEATURE columns never leave the GPU: a DeviceDB appends the rows of batch
runs (append) and of live streams' steps (attach / append_step: the step itself stores them, FD-2) on the device and hands them to train.prepare_db / train, dbstats.predict_db and knn.Knn.add_db; everything that is a string — file
name, part tag, time, labels — is kept here, one record per stored row, in the shape of the app's rows without `features`.

Not done here (DESIGN.md FD-1 / FD-2 "out of scope"): replacing a stored identity in place other than level 11's one row per stream
launch (a file the DB already holds is refused, as the app skips it: src/index.js:277), label editing, a DB spread over several
devices, '*' classes, a KNN store that grows by itself from the DB."""
import numpy as np

from . import capi
from .dbstats import js_number_str, to_fixed


def records(level, step, meta, kept, files):
    """The host record of every kept row, as the app would store it: {file, seg, time, true: None, pred: None, row}.  meta: the batch's
    row metadata [n][8] (level 11: the utterance metadata [n][4] = {clip, result, t_start, t_sum}); kept: the source row of every
    stored row; files: the file name of every clip; step = window_step in seconds.  seg is the part tag as the app's storage key holds it
    (String(si) at level 5, String(si + k / 100) at levels 12 / 13 with k the row's position in its callback, "0" at level 11); time is
    what the dispatcher hands over: two numbers at levels 5 / 11, the two toFixed(3) strings at 12 / 13."""
    pos = np.zeros(len(meta), np.int64)                  # k: the row's position among the rows of its (clip, si)
    if level in (12, 13):
        for r in range(1, len(meta)):
            if meta[r][0] == meta[r - 1][0] and meta[r][1] == meta[r - 1][1]:
                pos[r] = pos[r - 1] + 1
    out = []
    for i, r in enumerate(kept):
        m = meta[r]
        t0, td = int(m[2]) * step, (int(m[3]) + 1) * step
        if level == 5:
            seg, time = js_number_str(int(m[1])), [t0, td]
        elif level == 11:
            seg, time = "0", [t0, td]
        else:
            seg, time = js_number_str(int(m[1]) + int(pos[r]) / 100), [to_fixed(t0, 3), to_fixed(td, 3)]
        out.append({"file": files[int(m[0])], "seg": seg, "time": time, "true": None, "pred": None, "row": None})
    return out


class DeviceDB(capi.FeatDB):
    """One feature DB on an Analyzer's device: DeviceDB(analyzer, level, capacity) holds up to `capacity` rows of the level's width
    (53 at levels 5 / 13, 264 at 11, 23 at 12; capacity x width x 8 bytes of device memory, allocated once).  `records` is the host
    side, one dict per stored row ({file, seg, time, true, pred, row}: `row` is its DB row); set `true` / `pred` on them as on the app's rows."""

    def __init__(self, analyzer, level, capacity):
        width = capi.level_feature_count(level)
        if not width:
            raise ValueError(f"output_level {level} stores no feature rows (5, 11, 12 or 13 do)")
        super().__init__(analyzer, width, capacity)
        self.level = int(level)
        self.step = float(analyzer.config["window_step"]) / 1e3
        self.records = []
        self.files = set()
        self.streams, self.names, self.next_names = None, [], {}

    def attach(self, streams, names):
        """Every step of `streams` appends its rows to this DB on the device from now on (Streams.set_featdb, spec FD-2).  names: one
        per stream, the "file" of that stream's current launch; a name the DB already holds is refused, as append refuses files."""
        names = [str(f) for f in names]
        if len(names) != streams.n:
            raise ValueError(f"{len(names)} names for {streams.n} streams")
        again = [f for f in names if f in self.files] or [f for i, f in enumerate(names) if f in names[:i]]
        if again:
            raise ValueError(f"the DB already holds {again[0]!r}")
        streams.set_featdb(self)
        self.streams, self.names, self.next_names = streams, names, {}
        self.files.update(names)

    def detach(self):
        if self.streams is not None:
            self.streams.set_featdb(None)
        self.streams, self.names, self.next_names = None, [], {}

    def rename(self, i, name):
        """The name of stream i's NEXT launch: it takes effect in the step whose control byte carries START for it (append_step's ctl)."""
        name = str(name)
        if name in self.files:
            raise ValueError(f"the DB already holds {name!r}")
        if not 0 <= int(i) < len(self.names):
            raise ValueError(f"stream {i} of {len(self.names)}")
        self.files.discard(self.next_names.get(int(i)))
        self.next_names[int(i)] = name
        self.files.add(name)

    def append_step(self, rows, ctl=None):
        """After streams.collect(): rows is what it returned, ctl the control bytes the step was given (a stream with START takes the name
        set by rename).  Turns the step's kept / replaced lists into host records, shaped as append's, and returns them; at level 11 a
        replaced row's record is updated in place (and returned too)."""
        if self.streams is None:
            raise ValueError("append_step on a DB that is attached to no stream set")
        for i, cb in enumerate(ctl if ctl is not None else []):
            if int(cb) & 2 and i in self.next_names:         # WSA_STREAM_START
                self.names[i] = self.next_names.pop(i)
        d = self.streams.db_rows()
        meta = rows["utt_meta"] if self.level == 11 else rows["meta"]
        new = records(self.level, self.step, meta, d["kept"], self.names)
        for i, r in enumerate(new):
            r["row"] = d["first_row"] + i
        self.records += new
        out = list(new)
        for u, row in (d["replaced"] if d["replaced"] is not None else []):
            fresh = records(self.level, self.step, meta, [int(u)], self.names)[0]
            old = next(r for r in self.records if r["row"] == int(row))
            old.update(file=fresh["file"], seg=fresh["seg"], time=fresh["time"])
            out.append(old)
        return out

    def append(self, batch, files, stream=0):
        """Appends the batch's last run (one file name per clip) and returns the new records.  A file name the DB already holds is
        refused before anything is enqueued (the app skips such files, src/index.js:277 if_file_in_db)."""
        files = [str(f) for f in files]
        if len(files) != int(batch.info["n_clips"]):
            raise ValueError(f"{len(files)} file names for a batch of {batch.info['n_clips']} clips")
        again = [f for f in files if f in self.files] or [f for i, f in enumerate(files) if f in files[:i]]
        if again:
            raise ValueError(f"the DB already holds {again[0]!r}")
        # the metadata first: once the rows are in the DB nothing below can fail and leave the records behind the device's count
        meta = batch.utterance_meta(stream) if self.level == 11 else batch.row_meta(stream)
        if len(meta) and not (0 <= int(meta[:, 0].min()) and int(meta[:, 0].max()) < len(files)):
            raise ValueError(f"the run's metadata names a clip outside 0 .. {len(files) - 1}")
        first, kept = self.append_batch(batch, stream)
        new = records(self.level, self.step, meta, kept, files)
        for i, r in enumerate(new):
            r["row"] = first + i
        self.records += new
        self.files.update(files)
        return new

    def append_rows(self, db_rows, stream=0):
        """Host rows with `features` (an imported data_<db>.json): the features go to the device, the rest is kept as records."""
        feat = np.array([r["features"] for r in db_rows], np.float64).reshape(-1, self.width)
        first = self.append_host(feat, stream)
        new = [dict({k: v for k, v in r.items() if k != "features"}, row=first + i) for i, r in enumerate(db_rows)]
        self.records += new
        self.files.update(r["file"] for r in new)
        return new

    def close(self):
        if getattr(self, "streams", None) is not None and self.streams.h and self.h:      # the DB must outlive its attachment
            self.detach()
        super().close()

    def clear(self):
        super().clear()                                  # (refused while attached: detach, clear, attach)
        self.records, self.files = [], set()

    def to_rows(self, stream=0):
        """Ordinary db_rows (dbstats / train / js/featuredb.js's shape): one copy of the features to the host."""
        feat = self.copy_rows(0, None, stream)
        return [dict({k: v for k, v in r.items() if k != "row"}, features=[float(x) for x in f]) for r, f in zip(self.records, feat)]
