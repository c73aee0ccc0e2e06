// make_utterance_golden.js — fixture generator helper for output level 11's utterance histograms (K4).  TEST INFRASTRUCTURE, build-container only.
//
// Loads the reference's utterance module (inner module 7) out of dist/main.js AT RUN TIME by ref_driver.js's recipe (slice the inner bundle, expose
// its webpack require, shim window / document; nothing of the bundle is copied into this repository) and calls its own exported
// get_utterance_features(segments_ci, results[0 .. k]) for every result prefix of every case.  A result is [syllables_ci, frames per syllable] as the
// dispatcher pushes it; the frames come as float32 bytes (base64), so NaN and denormal inputs arrive as they are.  The function complains
// `Array sizes mismatch` whenever segments_ci is longer than the results (which it is in the dispatcher too, after a dropped segment) and goes on;
// anything else it says, or a null return, stops the generator.
//
// usage: node make_utterance_golden.js job.json out.json
//   job.json = {"bundle": ".../dist/main.js", "cases": [{"name", "segs": [[start, len]], "results": [{"syl": [[first, len]], "frames": base64}]}]}
//   out.json = {"node", "cases": [{"name", "rows": [[264 f64 as big-endian hex] per result prefix]}]}
'use strict';
const fs = require('fs');

function load_reference(bundle_path) {
  const b = fs.readFileSync(bundle_path);
  let src = b.slice(100, 114174).toString('latin1');
  src = src.slice(src.indexOf('function(module)'));
  if (src.indexOf('n(n.s=1)') < 0) throw new Error('bundle layout changed');
  src = src.replace('n(n.s=1)', '(globalThis.__fa_require=n,n(n.s=1))');
  global.window = { setTimeout: setTimeout, screen: {} };
  global.document = { getElementById: () => ({}) };
  const mod = { exports: {} };
  (0, eval)('(' + src + ')')(mod);
  return globalThis.__fa_require(7);
}

function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const um = load_reference(job.bundle);
  if (typeof um.get_utterance_features !== 'function') throw new Error('get_utterance_features is not exported');
  const buf = Buffer.alloc(8);
  const hex = x => { buf.writeDoubleBE(x); return buf.toString('hex'); };
  const cases = [];
  for (const c of job.cases) {
    const results = c.results.map(r => {
      const raw = Buffer.from(r.frames, 'base64');
      const all = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
      const frame = o => all.subarray(9 * o, 9 * o + 9);
      return [r.syl, r.syl.map(([st, sl]) => Array.from({ length: sl }, (_, o) => frame(st + o)))];
    });
    const rows = [];
    for (let k = 0; k < results.length; k++) {
      const said = [];
      const err = console.error; console.error = e => { said.push(String(e && e.message ? e.message : e)); };
      let v;
      try { v = um.get_utterance_features(c.segs, results.slice(0, k + 1)); } finally { console.error = err; }
      const other = said.filter(m => m !== 'Array sizes mismatch');
      if (v === null || other.length || v.length !== 264) throw new Error(c.name + ' prefix ' + k + ': ' + (v === null ? 'null' : v.length + ' numbers') + ' ' + other.join('; '));
      if ((said.length > 0) !== (c.segs.length !== k + 1)) throw new Error(c.name + ' prefix ' + k + ': the size complaint came ' + said.length + ' times');
      rows.push(Array.from(v, hex));
    }
    cases.push({ name: c.name, rows });
  }
  fs.writeFileSync(process.argv[3], JSON.stringify({ node: process.version, cases }));
}
main();
