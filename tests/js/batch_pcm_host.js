// batch_pcm_host.js — drives js/formantanalyzer.js's batch launches with clips in every encoding decode_wav hands on as bytes (spec PK-2) and
// with the same signals decoded on the host into Float32Arrays; prints both callback streams for tests/test_js_host_batch_pcm.py.
// job: {settings, fs, wavs: {name: path}, bad: path of a WAV nothing decodes, f32: [paths of raw float32], i16: [paths of raw int16]}
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function batch(clips) {
  const per = clips.map(() => []);
  await fa.LaunchBatch(clips, (si, label, t, f, clip) => per[clip].push([si, t, Array.from(f)]), clips.map((c, i) => ['clip' + i]));
  return per;
}
const raw = (p, T) => { const b = fs.readFileSync(p); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };

(async () => {
  fa.configure(Object.assign({}, fa._settings, { sample_rate: job.fs }, job.settings));
  const out = { wav: {}, floats: {}, kinds: {} };
  const names = Object.keys(job.wavs), files = names.map((n) => fs.readFileSync(job.wavs[n]));
  const decoded = files.map((b) => fa._decode_wav(b));
  names.forEach((n, i) => { out.kinds[n] = decoded[i].pcm16 ? 'pcm16' : decoded[i].pcm ? 'pcm' : decoded[i].format + '/' + decoded[i].channels; });
  const as_floats = decoded.map((c) => ({ pcm: fa._clip_floats(c), sampleRate: c.sampleRate }));
  // every encoding in one launch, as the files' buffers ...
  let per = await batch(files);
  names.forEach((n, i) => { out.wav[n] = per[i]; });
  // ... against the same signals as floats
  per = await batch(as_floats);
  names.forEach((n, i) => { out.floats[n] = per[i]; });
  // one file alone (a launch of one kind of packed clip), through LaunchAudioNodes as the app calls it
  const solo = [];
  await fa.LaunchAudioNodes(1, files[0], (si, label, t, f) => solo.push([si, t, Array.from(f)]), ['clip0'], true, false);
  out.solo = solo; out.solo_name = names[0];
  // play_offset / play_duration cut a packed clip on its frame boundaries, as they cut the floats
  const k = names.indexOf('pcm24');
  out.cut = []; out.cut_want = [];
  await fa.LaunchAudioNodes(1, files[k], (si, label, t, f) => out.cut.push([si, t, Array.from(f)]), [], true, false, 0.1, 1.0);
  await fa.LaunchAudioNodes(1, as_floats[k], (si, label, t, f) => out.cut_want.push([si, t, Array.from(f)]), [], true, false, 0.1, 1.0);
  // Float32Array and Int16Array clips mixed in one launch, against the Int16Array clips widened on the host
  const f32 = job.f32.map((p) => raw(p, Float32Array)), i16 = job.i16.map((p) => raw(p, Int16Array));
  const mixed = [f32[0], i16[0], f32[1], i16[1]];
  out.mixed = await batch(mixed);
  out.mixed_floats = await batch(mixed.map((c) => (c instanceof Int16Array ? Float32Array.from(c, (v) => v / 32768) : c)));
  // the pipelined launches take the same mixes
  const order = [];
  const perb = [[[], []], [[], []]];
  await fa.LaunchBatches([[files[0], f32[0]], [i16[0], files[1]]], (si, label, t, f, clip, b) => perb[b][clip].push([si, t, Array.from(f)]), [[['a'], ['b']], [['c'], ['d']]]);
  out.batches = perb;
  out.batches_want = [[out.floats[names[0]], out.mixed_floats[0]], [out.mixed_floats[1], out.floats[names[1]]]];
  // an object clip handed over directly, and a slice of it
  const obj = { packed: decoded[0].packed, format: decoded[0].format, channels: decoded[0].channels, sampleRate: decoded[0].sampleRate };
  out.object = (await batch([obj]))[0];
  out.bad = await fa.LaunchBatch([fs.readFileSync(job.bad)], () => {}).then(() => 'RESOLVED', (e) => String(e));
  out.bad_object = await fa.LaunchBatch([{ packed: new Uint8Array(64), format: 'pcm24', channels: 1, sampleRate: job.fs }], () => {}).then(() => 'RESOLVED', (e) => String(e));
  fa.shutdown();
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e && e.stack ? e.stack : String(e)); process.exit(1); });
