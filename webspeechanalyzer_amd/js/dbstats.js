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
function columns(samples, classLabels, ordinalLabels) {
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

module.exports = { heads, columns, assemble, lines, updatePredLabel, predictDB, statsTable, MAX_CLASSES, MAX_HEADS };
