// dbstats.js — the host side of predicting a labelled feature DB and of the app's results table (specification DS-1, K8): what the app's
// Predict button does around its models — src/neuralmodel.js:410-535 (predict_db_nn -> nn_db_results_handler), src/localstore.js:723-769
// (update_pred_label) and :498-627 (shows_stats_table).  Everything that is a string is resolved here, with the reference's own comparisons
// (strict indexOf for the class list, loose == between labels, truthiness of labels); the device (wsa_dbstats_*, through the addon's
// dbPredict / dbTable) sees indices and values, decides per row and counts.  columns / assemble / lines are pure and need no device.
'use strict';

const MAX_CLASSES = 256, MAX_HEADS = 8, MANY_CLASSES = 25;      // WSA_DBSTATS_MAX_CLASSES / _MAX_HEADS; localstore.js:560

function heads(classLabels, ordinalLabels) {
  const cats = (classLabels || []).map((h) => { const name = Object.keys(h)[0]; return { name, list: h[name] }; });
  const ords = (ordinalLabels || []).slice();
  if (cats.length > MAX_HEADS) throw 'statsTable: ' + cats.length + ' categorical heads (limit ' + MAX_HEADS + ')';
  if (ords.length > MAX_HEADS) throw 'statsTable: ' + ords.length + ' ordinal heads (limit ' + MAX_HEADS + ')';
  return { cats, ords };
}

// samples: [{time, truth, guess}] (featuredb.js Sample).  -> {n, durations, vocab, trueIdx, predIdx, trueVal, predVal, labels} as dbTable takes them
// legends (evaluateDB): {head name: the model's legend labels}, added to that head's vocabulary behind the labels found among the true pairs
function columns(samples, classLabels, ordinalLabels, legends) {
  const { cats, ords } = heads(classLabels, ordinalLabels), n = samples.length;
  if (n < 1) throw 'statsTable: a feature DB has at least one row';
  const durations = Float64Array.from(samples, (s) => parseFloat(s.time[1]));                  // localstore.js:534
  const trueIdx = new Int32Array(cats.length * n).fill(-1), predIdx = new Int32Array(cats.length * n).fill(-1);
  const trueVal = new Float64Array(ords.length * n).fill(NaN), predVal = new Float64Array(ords.length * n).fill(NaN);
  const labels = [];
  cats.forEach((head, h) => {
    const vocab = [];
    const slot = (v) => { let i = vocab.findIndex((e) => e == v); if (i < 0) { i = vocab.length; vocab.push(v); } return i; };   // loose, localstore.js:539
    const wildcard = head.list.indexOf('*') >= 0;
    samples.forEach((s, i) => {
      const v = s.truth && s.truth[0] ? s.truth[0][head.name] : undefined;
      if (v && (head.list.indexOf(v) >= 0 || wildcard)) trueIdx[h * n + i] = slot(v);           // localstore.js:523
    });
    for (const label of (legends && legends[head.name]) || []) slot(label);
    samples.forEach((s, i) => {
      const v = s.guess && s.guess[0] ? s.guess[0][head.name] : undefined;
      if (v) predIdx[h * n + i] = slot(v);                                                      // localstore.js:537
    });
    if (vocab.length > MAX_CLASSES) throw 'statsTable: head ' + head.name + ' has ' + vocab.length + ' distinct labels (limit ' + MAX_CLASSES + ')';
    if (!vocab.length) vocab.push('');
    labels.push(vocab);
  });
  ords.forEach((name, o) => {
    samples.forEach((s, i) => {
      const t = s.truth && s.truth[1] ? s.truth[1][name] : undefined, p = s.guess && s.guess[1] ? s.guess[1][name] : undefined;
      if (t !== undefined && t !== null) trueVal[o * n + i] = Number(t);                        // the device drops 0 and NaN (localstore.js:587, 593)
      if (p !== undefined && p !== null) predVal[o * n + i] = Number(p);
    });
  });
  return { n, names: cats.map((c) => c.name), ordNames: ords, durations, vocab: Uint32Array.from(labels, (v) => v.length), trueIdx, predIdx, trueVal, predVal, labels };
}

// counters: {cat [nCat][3], cls [sum V][5], ord [nOrd][5]} (the addon's dbTable) -> {cats, ords}
function assemble(col, counters) {
  const out = { cats: [], ords: [] };
  let off = 0;
  col.labels.forEach((vocab, h) => {
    const seen = [];
    vocab.forEach((label, v) => { const e = counters.cls.subarray((off + v) * 5, (off + v) * 5 + 5); if (e[0] > 0) seen.push({ label, count: e[0], correct: e[1], wrong: e[2], duration: e[3], first: e[4] }); });
    seen.sort((a, b) => a.first - b.first);                                                     // order of first appearance among the counted rows
    out.cats.push({ name: col.names[h], correct: counters.cat[h * 3], wrong: counters.cat[h * 3 + 1], blank: counters.cat[h * 3 + 2],
      classes: seen.map((e) => ({ label: e.label, count: e.count, duration: e.duration, correct: e.correct, wrong: e.wrong })) });
    off += vocab.length;
  });
  col.ordNames.forEach((name, o) => {
    const e = counters.ord.subarray(o * 5, o * 5 + 5);
    out.ords.push({ name, true_n: e[0], pred_n: e[1], min: e[2], max: e[3], sq_sum: e[4], rmse: Math.sqrt(e[1] > 0 ? e[4] / e[1] : 0) });   // localstore.js:602-603
  });
  return out;
}

// the panel's text, one item per <li> in the app's order, tags stripped and white space collapsed (localstore.js:558-610)
function lines(table) {
  const out = [];
  for (const h of table.cats) {
    const k = h.classes.length;
    out.push('Label: ' + h.name + ', Type: Class');
    out.push('Classes (' + k + '): ' + (k < MANY_CLASSES ? h.classes.map((c) => c.label) : 'Many'));
    out.push('Accuracy: ' + (h.correct * 100 / (h.correct + h.wrong)).toFixed(2) + '%');
    out.push('Correct: ' + h.correct + ', Wrong ' + h.wrong + ', NaN: ' + h.blank);
    if (k < MANY_CLASSES)
      for (const c of h.classes)
        out.push(c.label + ' : count: ' + c.count + ', minutes: ' + (c.duration / 60).toFixed(2) + ' ' + c.correct + ' ' + c.wrong + ' ' + (c.correct * 100 / (c.wrong + c.correct)).toFixed(2) + '%');
  }
  for (const o of table.ords) {
    out.push('Label: ' + o.name + ', Type: Ordinal');
    out.push('Range: ' + o.min + ' - ' + o.max);
    out.push('Samples: ' + o.true_n);
    out.push('Predicted: ' + o.pred_n);
    out.push('RMSE: ' + o.rmse.toFixed(3));
  }
  return out.map((s) => s.replace(/\s+/g, ' ').trim());
}

// localstore.js:723-769 on one sample: slot 0 when `label` names a categorical head, else slot 1 when it names an ordinal head; the pair is
// stored in every case, through JSON as the app's string storage does (NaN becomes null)
function updatePredLabel(sample, hd, label, value) {
  const pair = sample.guess ? sample.guess : [{}, {}];
  if (hd.cats.some((c) => c.name == label)) pair[0][label] = value;
  else if (hd.ords.some((name) => name == label)) pair[1][label] = value;
  sample.guess = JSON.parse(JSON.stringify(pair));
}

// device: {predict(handle, Float64Array [n][width], ords) -> Int32Array | Float64Array, table(col) -> counters} (formantanalyzer.js binds the addon)
function predictDB(device, featureDB, o) {
  if (!o || (o.type !== 'cats' && o.type !== 'ords') || !o.label) throw "predictDB(featureDB, {db, type: 'cats'|'ords', label, model | modelDir, classLabels, ordinalLabels})";
  const samples = featureDB.samples(o.db), hd = heads(o.classLabels, o.ordinalLabels);
  if (!samples.length) throw 'predictDB: no data for prediction';                              // neuralmodel.js:460
  const W = samples[0].vector.length;             // the DB's width: that of an ML level, and the model's input count
  if ([53, 264, 23].indexOf(W) < 0) throw 'predictDB: row 0 has ' + W + ' features; the models take level-5 / level-13 rows of 53 (or level-11 rows of 264, level-12 rows of 23)';
  const handle = o.model, regression = typeof handle.spec.outMin === 'number';
  if (handle.spec.units[0] !== W) throw 'predictDB: the model takes ' + handle.spec.units[0] + ' inputs; the rows of the DB have ' + W + ' features';
  const x = new Float64Array(samples.length * W);
  samples.forEach((s, r) => {
    if (s.vector.length !== W) throw 'predictDB: row ' + r + ' has ' + s.vector.length + ' features; the models take level-5 / level-13 rows of 53';
    for (let k = 0; k < W; k++) x[r * W + k] = Number(s.vector[k]);
  });
  if (regression !== (o.type === 'ords')) throw 'predictDB: a ' + o.type + ' prediction needs a ' + (o.type === 'ords' ? 'regression model' : 'classifier');
  const raw = device.predict(handle, x, o.type === 'ords');
  const preds = Array.from(raw, (v) => (o.type === 'ords' ? v : (v >= 0 ? handle.labels[v] : null)));
  samples.forEach((s, i) => updatePredLabel(s, hd, o.label, preds[i]));
  return preds;
}

function statsTable(device, featureDB, o) {
  const samples = featureDB.samples(o.db);
  const col = columns(samples, o.classLabels, o.ordinalLabels);
  if (!col.labels.length && !col.ordNames.length) return { cats: [], ords: [], lines: [] };
  const table = assemble(col, device.table(col));
  table.lines = lines(table);
  return table;
}

// ---- evaluation beyond the panel: specification EV-1 (DESIGN.md §3; K8e through the addon's dbEval; webspeechanalyzer_amd/dbstats.py is the same in Python)
const ratio = (a, b) => (b ? a / b : NaN);                        // 0 / 0 stays NaN, as the panel's Accuracy does
const pct = (x) => (x * 100).toFixed(2) + '%';

// matrix [V][V + 1] (column V: blank predictions) -> {recall [V], precision [V], uar}: recall[t] = m[t][t] / row t's sum, blanks included;
// precision[p] = m[p][p] / column p's sum; uar = the unweighted mean of the recalls of the classes that have a counted row
function confusionMetrics(m) {
  const V = m.length, rows = m.map((r) => r.reduce((a, b) => a + b, 0));
  const recall = m.map((r, t) => ratio(r[t], rows[t]));
  const precision = m.map((_, p) => ratio(m[p][p], m.reduce((a, r) => a + r[p], 0)));
  const have = recall.filter((_, t) => rows[t]);
  return { recall, precision, uar: ratio(have.reduce((a, b) => a + b, 0), have.length), V };
}

// conf: every head's [V][V + 1] one after the other (the addon's dbEval) -> [{name, labels, matrix, recall, precision, uar}]
function assembleConfusion(col, conf) {
  let off = 0;
  return col.labels.map((vocab, h) => {
    const V = vocab.length, matrix = [];
    for (let t = 0; t < V; t++) matrix.push(Array.from(conf.subarray(off + t * (V + 1), off + (t + 1) * (V + 1))));
    off += V * (V + 1);
    const k = confusionMetrics(matrix);
    return { name: col.names[h], labels: vocab.map(String), matrix, recall: k.recall, precision: k.precision, uar: k.uar };
  });
}

const AGREE = ['n', 'mean_true', 'mean_pred', 'var_true', 'var_pred', 'cov', 'ccc', 'pearson'];
function assembleAgreement(col, agree) {
  return col.ordNames.map((name, o) => { const e = { name }; AGREE.forEach((k, i) => { e[k] = agree[o * 8 + i]; }); return e; });
}

// text in the style of lines(): per head the matrix over the classes that occur (a counted row or a prediction), one line per true class with
// its recall, then the precisions and the UAR; 0 / 0 prints NaN as the panel does
function confusionLines(confusion) {
  const out = [];
  for (const h of confusion) {
    const m = h.matrix, V = h.labels.length, used = [];
    for (let v = 0; v < V; v++) if (m[v].reduce((a, b) => a + b, 0) || m.reduce((a, r) => a + r[v], 0)) used.push(v);
    out.push('Label: ' + h.name + ', Type: Class, Confusion');
    out.push('True \\ Predicted: ' + used.map((v) => h.labels[v]).concat(['NaN']).join(','));
    for (const t of used) out.push(h.labels[t] + ' : ' + used.concat([V]).map((p) => m[t][p]).join(' ') + ' recall: ' + pct(h.recall[t]));
    out.push('Precision: ' + used.map((p) => h.labels[p] + ' ' + pct(h.precision[p])).join(', '));
    out.push('UAR: ' + pct(h.uar));
  }
  return out.map((s) => s.replace(/\s+/g, ' ').trim());
}

function agreementLines(agreement) {
  const out = [];
  for (const o of agreement) {
    out.push('Label: ' + o.name + ', Type: Ordinal, Agreement');
    out.push('Pairs: ' + o.n);
    out.push('Mean: ' + o.mean_true.toFixed(3) + ' true, ' + o.mean_pred.toFixed(3) + ' predicted');
    out.push('Variance: ' + o.var_true.toFixed(3) + ' true, ' + o.var_pred.toFixed(3) + ' predicted, covariance ' + o.cov.toFixed(3));
    out.push('CCC: ' + o.ccc.toFixed(3));
    out.push('Pearson: ' + o.pearson.toFixed(3));
  }
  return out.map((s) => s.replace(/\s+/g, ' ').trim());
}

// {fileOfRow, callbackOfRow: Int32Array [n], names} from the samples' file and part tag: files numbered in order of first appearance, -1 without a
// file name; the callback is the integer part of the part tag (String(si), or String(si + k / 100) at levels 12 / 13), 0 where it is no number
function fileColumns(samples) {
  const names = [], index = new Map(), fileOfRow = new Int32Array(samples.length).fill(-1), callbackOfRow = new Int32Array(samples.length);
  samples.forEach((s, i) => {
    if (s.file !== null && s.file !== undefined && s.file !== '') {
      const key = String(s.file);
      if (!index.has(key)) { index.set(key, names.length); names.push(key); }
      fileOfRow[i] = index.get(key);
    }
    const si = parseFloat(s.part);
    callbackOfRow[i] = si === si && Math.abs(si) < 2147483648 ? Math.floor(si) : 0;
  });
  return { fileOfRow, callbackOfRow, names };
}

// the host rule for a file's label: per head that of the file's FIRST COUNTED row (trueIdx >= 0; a true value that is neither 0 nor NaN)
function fileTruths(col, fileOfRow, nFiles) {
  const n = col.n, nCat = col.labels.length, nOrd = col.ordNames.length;
  const idx = new Int32Array(nCat * nFiles).fill(-1), val = new Float64Array(nOrd * nFiles).fill(NaN);
  for (let i = n - 1; i >= 0; i--) {
    const f = fileOfRow[i];
    if (f < 0) continue;
    for (let h = 0; h < nCat; h++) if (col.trueIdx[h * n + i] >= 0) idx[h * nFiles + f] = col.trueIdx[h * n + i];
    for (let o = 0; o < nOrd; o++) { const v = col.trueVal[o * n + i]; if (v === v && v !== 0) val[o * nFiles + f] = v; }
  }
  return { idx, val };
}

function levelResult(col, t) {
  const table = assemble(col, t), confusion = assembleConfusion(col, t.conf), agreement = assembleAgreement(col, t.agree);
  return { table, confusion, agreement, lines: lines(table).concat(confusionLines(confusion), agreementLines(agreement)) };
}

// device: {evaluate(spec, catHandles, ordHandles) -> the addon's dbEval result} (formantanalyzer.js binds the addon and the model handles).
// o = {db, classLabels, ordinalLabels, models: {head name: model handle}, perFile (default true)}.  A named head is predicted on the device (every
// row, the samples' `pred` pairs written as predictDB does); the others are evaluated on the predictions the samples hold.  Returns
// {rows: {table, confusion, agreement, lines}, files: null | the same over the files plus names, sums, classes, values, folded}: the structure
// webspeechanalyzer_amd.dbstats.evaluate returns.
// Cross-validation (specification CV-1, js/crossval.js): with o.foldOfRow (Int32Array [n], -1: never held out) and o.nFolds, a head's entry of
// models may be an ARRAY of nFolds handles that share one legend — model k predicts the rows of fold k (K6f through the addon's dbEval), the rows
// of no fold stay blank.
function evaluateDB(device, featureDB, o) {
  o = o || {};
  const K = o.foldOfRow ? o.nFolds | 0 : 0, first = (m) => (Array.isArray(m) ? m[0] : m), members = (m) => (Array.isArray(m) ? m : [m]);
  const samples = featureDB.samples(o.db), hd = heads(o.classLabels, o.ordinalLabels), models = o.models || {};
  if (!samples.length) throw 'evaluateDB: a feature DB has at least one row';
  for (const name of Object.keys(models))
    if (!hd.cats.some((c) => c.name === name) && hd.ords.indexOf(name) < 0) throw 'evaluateDB: models names the head ' + name + '; the settings have ' + hd.cats.map((c) => c.name).concat(hd.ords);
  for (const name of Object.keys(models))
    if (Array.isArray(models[name]) && (models[name].length !== K || !K)) throw 'evaluateDB: head ' + name + ' has ' + models[name].length + ' models for ' + K + ' folds (foldOfRow, nFolds)';
  const legends = {};
  for (const c of hd.cats) if (models[c.name]) legends[c.name] = first(models[c.name]).labels;
  const col = columns(samples, o.classLabels, o.ordinalLabels, legends), n = col.n, nCat = col.labels.length, nOrd = col.ordNames.length;
  const empty = { table: { cats: [], ords: [] }, confusion: [], agreement: [], lines: [] };
  if (!nCat && !nOrd) return { rows: empty, files: null };
  const spec = { durations: col.durations, vocab: col.vocab, trueIdx: col.trueIdx, predIdx: col.predIdx, trueVal: col.trueVal, predVal: col.predVal, nFiles: 0 };
  const catHandles = col.names.map((name) => models[name] || null), ordHandles = col.ordNames.map((name) => models[name] || null);
  if (Object.keys(models).length) {
    const W = samples[0].vector.length;
    spec.width = W; spec.features = new Float64Array(n * W);
    samples.forEach((s, r) => {
      if (s.vector.length !== W) throw 'evaluateDB: row ' + r + ' has ' + s.vector.length + ' features, row 0 has ' + W;
      for (let k = 0; k < W; k++) spec.features[r * W + k] = Number(s.vector[k]);
    });
    const per = K || 1;                                            // ranges per ordinal head: one per member of a fold-wise head
    spec.catMaps = new Int32Array(nCat * 64).fill(-1); spec.ordRange = new Float64Array(nOrd * 2 * per);
    if (K) { spec.foldOfRow = Int32Array.from(o.foldOfRow); spec.nFolds = K; }
    catHandles.forEach((ms, h) => {
      if (!ms) return;
      for (const m of members(ms)) {
        if (typeof m.spec.outMin === 'number') throw 'evaluateDB: head ' + col.names[h] + ' needs a classifier';
        if (m.spec.units[0] !== W) throw 'evaluateDB: the model takes ' + m.spec.units[0] + ' inputs; the rows of the DB have ' + W + ' features';
      }
      first(ms).labels.forEach((label, c) => { spec.catMaps[h * 64 + c] = col.labels[h].findIndex((e) => e == label); });
    });
    ordHandles.forEach((ms, k) => {
      if (!ms) return;
      members(ms).forEach((m, f) => {
        if (typeof m.spec.outMin !== 'number') throw 'evaluateDB: head ' + col.ordNames[k] + ' needs a regression model';
        if (m.spec.units[0] !== W) throw 'evaluateDB: the model takes ' + m.spec.units[0] + ' inputs; the rows of the DB have ' + W + ' features';
        spec.ordRange[(k * per + f) * 2] = m.spec.outMin; spec.ordRange[(k * per + f) * 2 + 1] = m.spec.outMax;
      });
    });
  }
  let fc = null;
  if (o.perFile !== false) {
    fc = fileColumns(samples);
    if (fc.names.length) {
      const t = fileTruths(col, fc.fileOfRow, fc.names.length);
      Object.assign(spec, { nFiles: fc.names.length, fileOfRow: fc.fileOfRow, callbackOfRow: fc.callbackOfRow, fileTrueIdx: t.idx, fileTrueVal: t.val });
    } else fc = null;
  }
  const r = device.evaluate(spec, catHandles, ordHandles);
  catHandles.forEach((m, h) => { if (m) samples.forEach((s, i) => { const v = r.predIdx[h * n + i]; updatePredLabel(s, hd, col.names[h], v >= 0 ? col.labels[h][v] : null); }); });
  ordHandles.forEach((m, k) => { if (m) samples.forEach((s, i) => updatePredLabel(s, hd, col.ordNames[k], r.predVal[k * n + i])); });
  const out = { rows: levelResult(col, r.rows), files: null };
  if (fc && r.files) {
    const nf = fc.names.length, files = levelResult(col, r.files);
    files.names = fc.names; files.sums = {}; files.classes = {}; files.values = {}; files.folded = {};
    col.names.forEach((name, h) => {
      files.folded[name] = !!catHandles[h];                        // a head without a model has no probabilities to fold: its files are blank
      if (!catHandles[h]) return;
      const C = first(catHandles[h]).labels.length, s = r.files.sums[h];
      files.sums[name] = Array.from({ length: nf }, (_, f) => Array.from(s.subarray(f * C, (f + 1) * C)));
      files.classes[name] = Array.from(r.files.idx.subarray(h * nf, (h + 1) * nf), (v) => (v >= 0 ? String(col.labels[h][v]) : null));
    });
    col.ordNames.forEach((name, k) => { files.values[name] = Array.from(r.files.val.subarray(k * nf, (k + 1) * nf)); });
    out.files = files;
  }
  return out;
}

module.exports = { heads, columns, assemble, lines, updatePredLabel, predictDB, statsTable, confusionMetrics, assembleConfusion, assembleAgreement, confusionLines,
  agreementLines, fileColumns, fileTruths, evaluateDB, MAX_CLASSES, MAX_HEADS };
