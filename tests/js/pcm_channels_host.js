// pcm_channels_host.js — drives js/formantanalyzer.js's launches with configure({channel}) (spec PK-3) on interleaved WAVs and prints the callback
// streams beside those of mono launches of the same channels, for tests/test_js_host_pcm_channels.py.
// job: {settings, fs, stereo: path of a two-channel WAV, mono: [paths of one-channel WAVs holding its channels], mix: path of raw float32 holding its mix,
//       tri: path of a three-channel 24-bit WAV, tri_mix: raw float32 of its mix, tri_last: raw float32 of its channel 2}
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

// callbacks as [clip_index, labels, si, t, features], in the order they arrive
async function batch(clips, labels) {
  const got = [];
  await fa.LaunchBatch(clips, (si, label, t, f, clip) => got.push([clip, label, si, t, Array.from(f)]), labels);
  return got;
}
const raw = (p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const set = (channel) => fa.configure(Object.assign({}, fa._settings, { sample_rate: job.fs }, job.settings, { channel }));

(async () => {
  const out = {};
  const stereo = fs.readFileSync(job.stereo), tri = fs.readFileSync(job.tri), mono = job.mono.map((p) => fs.readFileSync(p));
  set('first');
  out.first = await batch([stereo, tri], [['call'], ['room']]);
  out.mono = await batch(mono, [['call', 'ch0'], ['call', 'ch1']]);
  out.mix_want = await batch([raw(job.mix), raw(job.tri_mix)], [['call'], ['room']]);
  out.last_want = await batch([raw(job.tri_last)], [['room']]);
  set('each');
  out.each = await batch([stereo, tri], [['call'], ['room']]);
  out.each_solo = [];
  await fa.LaunchAudioNodes(1, stereo, (si, label, t, f) => out.each_solo.push([label, si, t, Array.from(f)]), ['call'], true, false);
  set('mix');
  out.mix = await batch([stereo, tri], [['call'], ['room']]);
  set(1);
  out.one = await batch([stereo], [['call']]);
  set(2);
  out.two = await batch([tri], [['room']]);
  out.two_on_stereo = await fa.LaunchBatch([tri, stereo], () => {}).then(() => 'RESOLVED', (e) => String(e));
  out.batches = await fa.LaunchBatches([[stereo]], () => {}).then(() => 'RESOLVED', (e) => String(e));
  try { set('left'); out.bad_key = 'ACCEPTED'; } catch (e) { out.bad_key = String(e); }
  // decodePcm with a select
  const pcm = new Int16Array([100, -200, 300, -400, 500]);
  out.decode = { ch1: Array.from(fa.decodePcm('i16', pcm, 2, 1)), mix: Array.from(fa.decodePcm('i16', pcm, 2, 'mix')), ch0: Array.from(fa.decodePcm('i16', pcm, 2)) };
  try { fa.decodePcm('i16', pcm, 2, 2); out.decode.bad = 'ACCEPTED'; } catch (e) { out.decode.bad = String(e); }
  // streams: the stereo call as two streams that share one packed row, and its mix as a third, beside three float streams fed the decoded channels
  set('first');
  const call = fa._decode_wav(stereo).pcm16, frames = call.length / 2;
  const drive = (h, n, put) => {
    const sps = h.samplesPerStep, steps = Math.floor(frames / sps);
    for (let k = 0; k < steps; k++) {
      put(h, k * sps, sps);
      h.push(new Uint8Array(n).fill(fa.STREAM_ACTIVE | (k === 0 ? fa.STREAM_START : 0) | (k === steps - 1 ? fa.STREAM_STOP : 0)));
    }
    h.close();
  };
  const floats = [fa.decodePcm('i16', call, 2, 0), fa.decodePcm('i16', call, 2, 1), fa.decodePcm('i16', call, 2, 'mix')];
  out.stream_want = [[], [], []]; out.stream = [[], [], []];
  let h = fa.StreamOpen(3, job.fs, (si, label, t, f, s) => out.stream_want[s].push([si, t, Array.from(f)]), [], 4);
  drive(h, 3, (hh, j0, c) => floats.forEach((x, i) => hh.input.set(x.subarray(j0, j0 + c), i * hh.samplesPerStep)));
  h = fa.StreamOpen(3, job.fs, (si, label, t, f, s) => out.stream[s].push([si, t, Array.from(f)]), [], 4, 1024, { format: 'i16', channels: 2, select: [0, 1, 'mix'], source: [0, 0, 0] });
  drive(h, 3, (hh, j0, c) => hh.input.set(call.subarray(j0 * 2, (j0 + c) * 2), 0));          // one row, the source's
  try { fa.StreamOpen(2, job.fs, null, [], 4, 1024, { format: 'i16', channels: 2, select: [0, 2], source: [0, 0] }); out.stream_bad = 'ACCEPTED'; } catch (e) { out.stream_bad = String(e); }
  fa.shutdown();
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e && e.stack ? e.stack : String(e)); process.exit(1); });
