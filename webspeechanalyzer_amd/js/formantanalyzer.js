// formantanalyzer.js — drop-in for `require('formantanalyzer')` (formantanalyzer@1.1.6, the module
// /root/reference/src/index.js:9 loads) with the hot path running on an MI355X through libwsa.
//
// Same four exports, same argument meaning, same callback shapes, same string rejections as the
// reference's inner module 1 (ref dist/main.js:2 @B2750-5843):
//   configure(cfg)                                                         ref @B3292
//   LaunchAudioNodes(context_source, source_obj, callback, file_labels=[], offline=false,
//                    test_play=true, play_offset=null, play_duration=null) -> Promise<true>   ref @B4469
//   StopAudioNodes(reason)                                                 ref @B5699
//   set_predicted_label_for_segment(si, idx, label)                        ref @B21711
// Node has no Web Audio, so context_source 1 (file) takes the audio as a WAV ArrayBuffer/Buffer, a
// Float32Array (+ sampleRate option) or {pcm, sampleRate}; sources 2 (element) and 3 (microphone)
// reject with "Invalid audio source" like the reference does for anything it cannot play.
// Extension for batch work (BASELINE configs 2-4): LaunchBatch(clips, callback, labels).
'use strict';
const path = require('path');

let native = null;
function addon() {
  if (!native) {
    // no fallback: without the addon + libwsa.so (+ a gfx950 GPU at create time) this throws
    native = require(path.join(__dirname, '..', 'lib', 'wsa_napi.node'));
  }
  return native;
}

// ref @B2965 — the library's own defaults (output_level 4 there; plot keys accepted and ignored)
const settings = {
  plot_enable: false, spec_type: 1, output_level: 4, plot_len: 200, f_min: 50, f_max: 4000,
  N_fft_bins: 256, N_mel_bins: 128, window_width: 25, window_step: 25, pause_length: 200,
  min_seg_length: 50, auto_noise_gate: true, voiced_max_dB: 100, voiced_min_dB: 10, plot_lag: 1,
  pre_norm_gain: 1000, high_f_emph: 0, plot_canvas: null, canvas_width: 200, canvas_height: 100,
  sample_rate: 16000, device: 0,          // ours: rate assumed for raw Float32Array input; GPU ordinal
  devices: null,                          // ours: GPU ordinals a LaunchBatch is sharded over (contiguous clip shards, one context and one worker thread each)
  gather: null,                           // ours: collect the shards' feature rows on the first device with one RCCL exchange and copy them to the host once
                                          // (levels 5 / 13; null = whenever more than one device is configured, true / false = always / never)
  resample_to: 0,                         // ours: analysis rate the audio is converted to first (0 = analyse at its own rate); 48000 = what the
                                          // reference's offline path gets from the browser (OfflineAudioContext at 48 kHz, ref @B18769)
  channel: 'first',                       // ours: what LaunchBatch / LaunchAudioNodes analyse of an interleaved clip (spec PK-3): 'first' (channel 0), 'mix' (the mono
                                          // mix, what a one-channel Web Audio context makes of the source), a channel number, or 'each' (every channel an
                                          // analysis of its own; the clip's bytes travel once)
};

// ref @B3292: truthy-merge, except the five keys tested with `null !==` (0 / false are honoured,
// and an absent key overwrites with undefined — the app always passes all keys, src/index.js:370-390)
function configure(e) {
  // (our key `channel` is checked before anything is taken over: a refused call changes no setting)
  if (e.channel !== undefined && e.channel !== null && !(e.channel === 'first' || e.channel === 'mix' || e.channel === 'each' || (Number.isInteger(e.channel) && e.channel >= 0 && e.channel < 64)))
    throw "channel: 'first', 'mix', 'each' or a channel number 0 .. 63";
  if (null !== e.spec_type) settings.spec_type = e.spec_type;
  if (e.output_level) settings.output_level = e.output_level;
  if (null !== e.f_min) settings.f_min = e.f_min;
  if (e.f_max) settings.f_max = e.f_max;
  if (e.N_fft_bins) settings.N_fft_bins = e.N_fft_bins;
  if (e.N_mel_bins) settings.N_mel_bins = e.N_mel_bins;
  if (e.window_width) settings.window_width = e.window_width;
  if (e.window_step) settings.window_step = e.window_step;
  if (e.pre_norm_gain) settings.pre_norm_gain = e.pre_norm_gain;
  if (null !== e.high_f_emph) settings.high_f_emph = e.high_f_emph;
  if (e.pause_length) settings.pause_length = e.pause_length;
  if (e.min_seg_length) settings.min_seg_length = e.min_seg_length;
  if (null !== e.auto_noise_gate) settings.auto_noise_gate = e.auto_noise_gate;
  if (e.voiced_max_dB) settings.voiced_max_dB = e.voiced_max_dB;
  if (null !== e.voiced_min_dB) settings.voiced_min_dB = e.voiced_min_dB;
  if (e.sample_rate) settings.sample_rate = e.sample_rate;
  if (e.device !== undefined && e.device !== null) settings.device = e.device;
  if (e.devices !== undefined) settings.devices = Array.isArray(e.devices) && e.devices.length > 0 ? e.devices.slice() : null;
  if (e.resample_to !== undefined && e.resample_to !== null) settings.resample_to = e.resample_to;
  if (e.gather !== undefined) settings.gather = e.gather === null ? null : !!e.gather;
  if (e.channel !== undefined && e.channel !== null) settings.channel = e.channel;
  settings.plot_enable = false;            // no canvas under Node
}

function native_config() {
  const c = {};
  for (const k of ['spec_type', 'output_level', 'f_min', 'f_max', 'N_fft_bins', 'N_mel_bins', 'window_width',
    'window_step', 'pause_length', 'min_seg_length', 'auto_noise_gate', 'voiced_max_dB', 'voiced_min_dB',
    'pre_norm_gain', 'high_f_emph']) c[k] = settings[k];
  return c;
}

// ---- minimal RIFF/WAVE reader (PCM 8/16/24/32-bit and float32, also WAVE_FORMAT_EXTENSIBLE); channel 0 is analysed —
// what a worklet reading inputs[0][0] sees (the reference hands the decoded buffer straight to its worklet node, ref @B20010;
// the worklet itself is not in the tree, so this choice belongs to the front-end specification FE-1)
const LITTLE_ENDIAN = new Uint8Array(new Uint16Array([1]).buffer)[0] === 1;
function decode_wav(buf) {
  const b = Buffer.isBuffer(buf) ? buf : Buffer.from(buf);
  if (b.length < 44 || b.toString('ascii', 0, 4) !== 'RIFF' || b.toString('ascii', 8, 12) !== 'WAVE') throw 'Unable to decode audio data';
  let pos = 12, fmt = null, data = null;
  while (pos + 8 <= b.length) {
    const id = b.toString('ascii', pos, pos + 4), len = b.readUInt32LE(pos + 4);
    if (id === 'fmt ') {
      fmt = { tag: b.readUInt16LE(pos + 8), ch: b.readUInt16LE(pos + 10), rate: b.readUInt32LE(pos + 12), bits: b.readUInt16LE(pos + 22) };
      if (fmt.tag === 0xfffe && len >= 26) fmt.tag = b.readUInt16LE(pos + 8 + 24);          // extensible: first word of the SubFormat GUID
    }
    else if (id === 'data') { data = b.subarray(pos + 8, Math.min(b.length, pos + 8 + len)); break; }
    pos += 8 + len + (len & 1);
  }
  if (!fmt || !data) throw 'Unable to decode audio data';
  const bytes = fmt.bits >> 3, n = Math.floor(data.length / (bytes * fmt.ch));
  // the encodings the browser's decodeAudioData takes from a WAV: integer PCM (1), IEEE float (3), G.711 A-law (6) and mu-law (7), plain or extensible
  const format = fmt.tag === 1 ? { 8: 'u8', 16: 'i16', 24: 'i24', 32: 'i32' }[fmt.bits] : fmt.tag === 3 ? { 32: 'f32', 64: 'f64' }[fmt.bits]
    : fmt.tag === 6 && fmt.bits === 8 ? 'alaw' : fmt.tag === 7 && fmt.bits === 8 ? 'mulaw' : undefined;
  if (fmt.ch < 1 || !format) throw 'Unable to decode audio data';
  if (format === 'i16' && LITTLE_ENDIAN) {
    // 16-bit PCM (what WAV files usually hold) is not decoded here at all: the data chunk goes to the device as it is — interleaved
    // channels and all, half the PCIe bytes of floats — and libwsa converts channel 0 there (x / 32768, exact in fp32)
    const bytes_used = n * fmt.ch * 2;
    const aligned = (data.byteOffset & 1) === 0 ? data : Buffer.from(data.subarray(0, bytes_used));      // an odd offset needs one memcpy
    return { pcm16: new Int16Array(aligned.buffer, aligned.byteOffset, n * fmt.ch), channels: fmt.ch, sampleRate: fmt.rate };
  }
  // every other encoding likewise (spec PK-2): a view of the data chunk's whole frames, whatever its address, and the name of what it holds —
  // no loop over the samples and no copy here; libwsa turns channel 0 into floats on the device (clip_floats does it on the host for who needs floats)
  return { packed: new Uint8Array(data.buffer, data.byteOffset, n * fmt.ch * bytes), format, channels: fmt.ch, sampleRate: fmt.rate };
}

// a clip = { pcm: Float32Array (mono), sampleRate }, { pcm16: Int16Array (interleaved over `channels`), channels, sampleRate } or
// { packed: Uint8Array (the bytes a file holds, little-endian, interleaved over `channels`), format: a name of CLIP_FORMATS, channels, sampleRate }
const CLIP_FORMATS = { f32: [0, 4], i16: [1, 2], mulaw: [2, 1], alaw: [3, 1], u8: [8, 1], i24: [9, 3], i32: [10, 4], f64: [11, 8] };       // name: [WSA_PCM_* of include/wsa.h, bytes per sample]
function to_pcm(source_obj) {
  if (source_obj instanceof Float32Array) return { pcm: source_obj, sampleRate: settings.sample_rate };
  if (source_obj instanceof Int16Array) return { pcm16: source_obj, channels: 1, sampleRate: settings.sample_rate };
  if (source_obj && source_obj.pcm instanceof Float32Array) return { pcm: source_obj.pcm, sampleRate: source_obj.sampleRate || settings.sample_rate };
  if (source_obj && source_obj.pcm16 instanceof Int16Array) return { pcm16: source_obj.pcm16, channels: source_obj.channels || 1, sampleRate: source_obj.sampleRate || settings.sample_rate };
  if (source_obj && source_obj.packed instanceof Uint8Array) {
    const ch = source_obj.channels || 1;
    if (!Object.prototype.hasOwnProperty.call(CLIP_FORMATS, source_obj.format) || !(ch >= 1 && ch <= 64)) throw 'Invalid audio source';
    return { packed: source_obj.packed, format: source_obj.format, channels: ch, sampleRate: source_obj.sampleRate || settings.sample_rate };
  }
  if (source_obj instanceof ArrayBuffer || Buffer.isBuffer(source_obj) || ArrayBuffer.isView(source_obj)) return decode_wav(source_obj);
  throw 'Invalid audio source';
}

function g711_linear(code, mulaw) {    // ITU-T G.711 code -> 16-bit linear value (spec PK-1)
  if (mulaw) { const u = ~code & 0xff, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84; return (u & 0x80 ? -mag : mag) | 0; }      // (| 0: codes 0x7F and 0xFF give +0, as the integer arithmetic of the library does)
  const a = (code ^ 0x55) & 0xff, e = (a >> 4) & 7, m = a & 15, mag = e === 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
  return a & 0x80 ? mag : -mag;
}
function clip_floats(c) {              // channel 0 of a clip as floats, decoded here on the host (for callers that need the floats: the launches send the bytes)
  if (c.pcm) return c.pcm;
  const ch = c.channels, n = clip_length(c), x = new Float32Array(n);
  if (c.pcm16) { for (let i = 0; i < n; i++) x[i] = c.pcm16[i * ch] / 32768; return x; }
  const d = Buffer.from(c.packed.buffer, c.packed.byteOffset, c.packed.length), step = ch * CLIP_FORMATS[c.format][1];
  for (let i = 0; i < n; i++) {
    const o = i * step;
    switch (c.format) {
      case 'f32': x[i] = d.readFloatLE(o); break;
      case 'f64': x[i] = d.readDoubleLE(o); break;
      case 'i16': x[i] = d.readInt16LE(o) / 32768; break;
      case 'u8': x[i] = (d[o] - 128) / 128; break;
      case 'i24': x[i] = d.readIntLE(o, 3) / 8388608; break;
      case 'i32': x[i] = d.readInt32LE(o) / 2147483648; break;
      default: x[i] = g711_linear(d[o], c.format === 'mulaw') / 32768;
    }
  }
  return x;
}
function clip_slice(c, a, b) {         // samples [a, b) of a clip (bufferSource.start(0, offset, duration))
  if (c.pcm) return { pcm: c.pcm.subarray(a, Math.min(b, c.pcm.length)), sampleRate: c.sampleRate };
  const ch = c.channels, n = clip_length(c);
  if (c.pcm16) return { pcm16: c.pcm16.subarray(a * ch, Math.min(b, n) * ch), channels: ch, sampleRate: c.sampleRate };
  const step = ch * CLIP_FORMATS[c.format][1];
  return { packed: c.packed.subarray(a * step, Math.min(b, n) * step), format: c.format, channels: ch, sampleRate: c.sampleRate };
}
function clip_length(c) {
  return c.pcm ? c.pcm.length : c.pcm16 ? Math.floor(c.pcm16.length / c.channels) : Math.floor(c.packed.length / (c.channels * CLIP_FORMATS[c.format][1]));
}
// one batch of clips to the addon.  Clips of one kind keep their call (all floats: wsa_batch_run_host, all Int16Array: wsa_batch_run_host_i16); any
// other mix travels as the bytes the clips hold, every clip with its own format and channel count, and is unpacked on the device
// (wsa_batch_run_host_packed, spec PK-2): Float32Array clips as 'f32', Int16Array clips as 'i16' — views, nothing is converted or copied here
// With configure({channel}) other than 'first' the clips are analyses (expand_channels): every one travels as bytes with the channel it takes (or the mix) and
// the analysis whose bytes it reads — the first of its file in this batch, so a file's bytes travel once (wsa_batch_run_host_channels, spec PK-3)
const CHANNEL_MIX = 0xFFFFFFFF;
function submit_clips(nat, ctx, clips, fs, fs_an, defer, extra) {
  if (clips.some((c) => c.select !== undefined)) {
    const bytes_of = (a) => new Uint8Array(a.buffer, a.byteOffset, a.byteLength);
    const first = new Map();                   // file -> the first analysis of it in this batch
    clips.forEach((c, i) => { if (!first.has(c.origin)) first.set(c.origin, i); });
    return nat.processBatch(ctx, clips.map((c) => (c.pcm ? bytes_of(c.pcm) : c.pcm16 ? bytes_of(c.pcm16) : c.packed)), fs, settings.output_level, fs_an,
      Uint32Array.from(clips, (c) => (c.pcm ? 1 : c.channels)), defer, extra[0],
      Int32Array.from(clips, (c) => (c.pcm ? CLIP_FORMATS.f32[0] : c.pcm16 ? CLIP_FORMATS.i16[0] : CLIP_FORMATS[c.format][0])),
      Uint32Array.from(clips, (c) => c.select), Uint32Array.from(clips, (c) => first.get(c.origin)));
  }
  if (clips.every((c) => c.pcm16)) return nat.processBatch(ctx, clips.map((c) => c.pcm16), fs, settings.output_level, fs_an, Uint32Array.from(clips, (c) => c.channels), defer, ...extra);
  if (clips.every((c) => c.pcm)) return nat.processBatch(ctx, clips.map((c) => c.pcm), fs, settings.output_level, fs_an, undefined, defer, ...extra);
  const bytes_of = (a) => new Uint8Array(a.buffer, a.byteOffset, a.byteLength);
  return nat.processBatch(ctx, clips.map((c) => (c.pcm ? bytes_of(c.pcm) : c.pcm16 ? bytes_of(c.pcm16) : c.packed)), fs, settings.output_level, fs_an,
    Uint32Array.from(clips, (c) => (c.pcm ? 1 : c.channels)), defer, extra[0],
    Int32Array.from(clips, (c) => (c.pcm ? CLIP_FORMATS.f32[0] : c.pcm16 ? CLIP_FORMATS.i16[0] : CLIP_FORMATS[c.format][0])));
}

// configure({channel}): the launch's clips -> its analyses.  'first': the clips as they are (channel 0, the calls of before).  'mix' / a number: one analysis per
// clip.  'each': a clip of C channels becomes C analyses in channel order, labelled labels[clip].concat('ch' + c).  -> { list, labels }
function expand_channels(list, labels) {
  const want = settings.channel;
  if (want === 'first') return { list, labels };
  const out = [], lab = [];
  list.forEach((c, i) => {
    const ch = c.pcm ? 1 : c.channels;
    const picks = want === 'each' ? Array.from({ length: ch }, (_, k) => k) : [want === 'mix' ? CHANNEL_MIX : want];
    for (const k of picks) {
      out.push(Object.assign({}, c, { select: k, origin: c }));
      lab.push(want === 'each' ? (labels[i] || []).concat('ch' + k) : (labels[i] || []));
    }
  });
  return { list: out, labels: lab };
}

// ---- contexts are kept across launches (creating one is cheap, but the planned batch the addon keeps with it is not: GBs of
// work space); a launch with other settings or devices replaces them, shutdown() releases them
let ctx_cache = { key: null, ctxs: [] };
function contexts_for(nat, devs) {
  const key = JSON.stringify([native_config(), devs]);
  if (ctx_cache.key !== key) {
    drop_contexts(nat);
    const ctxs = [];
    try { for (const d of devs) ctxs.push(nat.create(native_config(), d)); }
    catch (e) { for (const c of ctxs) { try { nat.destroy(c); } catch (e2) { /* first error wins */ } } throw e; }
    ctx_cache = { key, ctxs };
  }
  return ctx_cache.ctxs;
}
function drop_contexts(nat) {
  for (const c of ctx_cache.ctxs) knn_natives.delete(c);
  for (const c of ctx_cache.ctxs) { try { nat.destroy(c); } catch (e) { /* still in use by a failed launch's stragglers: left to process exit */ } }
  ctx_cache = { key: null, ctxs: [] };
}
function shutdown() {
  if (playing) return;
  if (native) { drop_contexts(native); drop_pipe_contexts(native); }
  release_models();
}

// ---- page-locked clip memory (ours; no counterpart in the reference, which hands the browser a file's ArrayBuffer, src/index.js:291).  A clip that
// lies in an ArrayBuffer from allocPinned goes to the GPU by DMA at the PCIe link's rate; a clip in ordinary memory is staged by the runtime
// through its own pinned buffers first (about half that rate).  A host that reads many files reads them into views of such buffers:
//     const ab = fa.allocPinned(n * 2); fs.readSync(fd, Buffer.from(ab), ...); clips.push({ pcm16: new Int16Array(ab), channels: 1, sampleRate })
// LaunchBatch / LaunchAudioNodes accept pinned and ordinary clips alike.  The memory goes back when the ArrayBuffer is collected.
function allocPinned(bytes) {
  const nat = addon();
  const ctxs = contexts_for(nat, settings.devices ? settings.devices.slice() : [settings.device]);
  return nat.allocPinned(ctxs[0], bytes);
}

// the page-locked memory behind an ArrayBuffer of allocPinned goes back now — at a moment the caller chooses, not whenever the garbage collector finalizes the buffer
// (releasing page-locked memory synchronises the device) — and the ArrayBuffer is detached.  No launch may still be reading it.
function freePinned(ab) { return addon().freePinned(ab); }

// ---- module state: one analysis at a time, like the reference's global nodes (ref @B4554)
let playing = false, stop_requested = false;
let labels_per_segment = [];
const open_streams = new Set();

// ---- the app's syllable classifier (ref src/index.js:56 -> src/prediction.js:47; K6 / K6b, include/wsa.h "Syllable classification").
// loadModel(dir | {model, meta, weights}) parses the files the app ships in dist/nnmodel/<db>/cats_<label>/ (model.json: a Sequential stack of
// Dense layers + weightsManifest; model.weights.bin: float32 kernels [in][out] and biases; model_meta.json: input ranges, output legend) and
// returns a handle; setPredictionModel(handle | null, on_prediction) makes every level-13 launch classify its syllables on the GPU and call
//     on_prediction(si, [label, confidence], clip_index, per_syllable)
// right after each segment's callback — the first two arguments are what the app's callback_after_pred receives (ref prediction.js:70), so
// `(si, lc) => fa.set_predicted_label_for_segment(si, 1, lc)` is the app's wiring (ref src/index.js:102-104); per_syllable is what ml5's
// classifyMultiple returned for the segment's syllables (for ONE syllable: that syllable's sorted list itself).  Callbacks whose durations
// sum to 0 get no on_prediction (the reference predicts nothing there).  The per-clip accumulator behind the app's meters (Label_conf_all,
// reset per launch) is on the resolved result of LaunchBatch / LaunchBatches as `meters`.  With no model set nothing changes.
//
// setPredictionModels([handles], on_prediction) is the same with ALL of the app's model DBs (ref src/prediction.js:12 `available_DBs`, in that order;
// K6e, include/wsa.h "Ensembles"): every level-13 launch classifies with all of them in one pass and calls
//     on_prediction(si, [label, confidence], clip_index, detail)
// where the first two arguments are what callback_after_pred receives with all DBs active (the label of the DB with the largest segment sum,
// ref prediction.js:156-168) and detail = {db, per_db: [{label, confidence, per_syllable}], min_entropy_db, entropy, meters}: the index of the
// winning DB (null with the label), every DB's own pair and classifyMultiple result, and what plot_prediction_meters draws after the
// callback (ref prediction.js:172-215) — the DB whose accumulator is the most decided, `1 - max / sum` of its Label_conf_all, and each label's
// share of that sum in Object.keys order.  The device reports no min_entropy_db for a launch in which no accumulator has exceeded 0; the
// reference keeps the previous launch's DB there (it never resets the variable), so this module carries the last one across launches in dispatch
// order, as the reference's one global does: min_entropy_db is null only before any launch had one; entropy is NaN and meters is {} while the
// carried DB's accumulator of this launch is empty.  The resolved result's `meters` holds, per clip, the meters of the clip's own
// min_entropy_db ({} for a clip without one), `min_entropy_db` the clips' DBs (null: none) and `shown_min_entropy_db` the carried one.  setPredictionModel and setPredictionModels replace each other.
const ACT = { linear: 0, relu: 1, sigmoid: 2, tanh: 3, softmax: 4 };
const loaded_models = new Set();
let prediction = null;                  // {model, on_prediction} | {models, on_prediction, state: {min_db}} (an ensemble; state: the carried min_entropy_db)
function parse_model(mj, meta, weights) {
  const topo = mj.modelTopology, layers = topo && topo.config && (Array.isArray(topo.config) ? topo.config : topo.config.layers);
  if (!topo || topo.class_name !== 'Sequential' || !Array.isArray(layers)) throw 'loadModel: model.json is not a Sequential model';
  const man = [].concat(...(mj.weightsManifest || []).map((g) => g.weights));
  if (layers.length < 1 || man.length !== 2 * layers.length) throw 'loadModel: weightsManifest does not list a kernel and a bias per layer';
  const act = layers.map((l, i) => {
    if (l.class_name !== 'Dense') throw 'loadModel: layer ' + i + ' is ' + l.class_name + '; only Dense layers are supported';
    const a = l.config.activation || 'linear';
    if (!(a in ACT)) throw 'loadModel: layer ' + i + ' has activation ' + a;
    return ACT[a];
  });
  const bytes = man.reduce((t, w) => t + 4 * w.shape.reduce((x, y) => x * y, 1), 0);
  if (weights.byteLength !== bytes) throw 'loadModel: model.weights.bin holds ' + weights.byteLength + ' bytes, the weightsManifest needs ' + bytes;
  const buf = new Uint8Array(weights.buffer ? weights.buffer.slice(weights.byteOffset, weights.byteOffset + weights.byteLength) : weights);
  const units = [man[0].shape[0]], kernels = [], biases = [];
  let off = 0;
  for (let i = 0; i < layers.length; i++) {
    const ks = man[2 * i].shape, bs = man[2 * i + 1].shape;
    if (ks.length !== 2 || ks[0] !== units[i] || bs[0] !== ks[1]) throw 'loadModel: layer ' + i + ' shapes do not chain';
    kernels.push(new Float32Array(buf.slice(off, off + 4 * ks[0] * ks[1]).buffer)); off += 4 * ks[0] * ks[1];
    biases.push(new Float32Array(buf.slice(off, off + 4 * bs[0]).buffer)); off += 4 * bs[0];
    units.push(ks[1]);
  }
  const W = units[0];                   // the row width of an ML level: 53 (levels 5 and 13), 264 (level 11) or 23 (level 12)
  if (W !== 53 && W !== 264 && W !== 23) throw 'loadModel: the model takes ' + W + ' inputs; the feature rows have 53 (output_level 5 and 13), 264 (output_level 11) or 23 (output_level 12)';
  const inMin = new Float64Array(W), inMax = new Float64Array(W);
  for (let k = 0; k < W; k++) { const r = meta.inputs[String(k)]; inMin[k] = r.min; inMax[k] = r.max; }
  const out = meta.outputs.y || Object.values(meta.outputs)[0];
  if (out && !out.legend && typeof out.min === 'number' && typeof out.max === 'number') {       // a regression model (ords_<label>): the output's range, no legend
    if (units[units.length - 1] !== 1 || act[act.length - 1] === ACT.softmax) throw 'loadModel: model_meta.json describes a regression output; the model does not end in one non-softmax unit';
    if (!(out.max !== out.min) || !isFinite(out.min) || !isFinite(out.max)) throw 'loadModel: model_meta.json: output range ' + out.min + ' .. ' + out.max;
    return { units: Int32Array.from(units), activation: Int32Array.from(act), kernels, biases, inMin, inMax, labels: [], outMin: out.min, outMax: out.max };
  }
  const labels = Object.keys(out.legend);
  return { units: Int32Array.from(units), activation: Int32Array.from(act), kernels, biases, inMin, inMax, labels };
}
function loadModel(src) {
  const fs = require('fs');
  let mj, meta, weights;
  if (typeof src === 'string') {
    mj = JSON.parse(fs.readFileSync(path.join(src, 'model.json'), 'utf8'));
    meta = JSON.parse(fs.readFileSync(path.join(src, 'model_meta.json'), 'utf8'));
    const paths = [].concat(...(mj.weightsManifest || []).map((g) => g.paths || []));
    weights = Buffer.concat((paths.length ? paths : ['model.weights.bin']).map((p) => fs.readFileSync(path.join(src, path.basename(p)))));
  } else if (src && src.model && src.meta && src.weights) {
    mj = typeof src.model === 'string' ? JSON.parse(src.model) : src.model;
    meta = typeof src.meta === 'string' ? JSON.parse(src.meta) : src.meta;
    weights = src.weights;
  } else throw 'loadModel(dir | {model, meta, weights})';
  const h = { spec: parse_model(mj, meta, weights), natives: new Map(), released: false };
  h.labels = h.spec.labels.slice();
  loaded_models.add(h);
  return h;
}
// ---- training (ref src/neuralmodel.js:163-403 train_nn + download_nn_model; K7 / specification TR-1, include/wsa.h "Training").
// trainModel({features: [[53 numbers]] (or rows of 264 / 23 numbers: the vectors of output_level 11 / 12), labels, classes, options, epochs, batchSize, seed, onEpoch}) -> Promise of a model handle that
// setPredictionModel / setPredictionModels accept.  `options` is the app's options JSON ({layers, learningRate}); onEpoch(epoch, {loss, acc,
// val_loss, val_acc}) mirrors ml5's whileTraining.  The selection, balancing, seeded initial weights and epoch orders live in trainmodel.js;
// `init` ({kernels, biases}) and `orders` (Uint32Array [epochs][nTrain]) replace the seeded ones.  The epochs run off the JS thread.
// The handle also carries `history` ([{loss, acc, val_loss, val_acc}] per epoch).  saveModel(handle, dir) writes the three files loadModel reads.
function plan_train_model(o) {        // -> {spec, job, onEpoch}: what the addon's train takes
  const tm = require('./trainmodel.js');
  const opt = Object.assign({}, tm.DEFAULT_OPTIONS, o.options || {});
  const data = o.db ? device_db_data(o.db, tm.select(o.labels, o.classes), o.labels.length) : tm.prepare(o.features, o.labels, o.classes);
  if (o.legend) {                       // a legend given from outside (crossValidate: the one legend of all folds), y re-indexed against it
    const legend = o.legend.map(String), own = data.legend;
    data.y = Int32Array.from(data.y, (j) => { const c = legend.indexOf(own[j]); if (c < 0) throw 'trainModel: the legend lacks the class ' + own[j]; return c; });
    data.legend = legend;
  }
  const st = tm.stack(opt.layers, data.legend.length, data.width), epochs = o.epochs === undefined ? 10 : o.epochs | 0, seed = o.seed | 0;
  const sp = tm.split(data.y.length, o.validationSplit);
  const init = o.init || tm.glorotInit(Array.from(st.units), seed);
  const spec = { units: st.units, activation: st.activation, kernels: init.kernels.map((k) => Float32Array.from(k)), biases: init.biases.map((b) => Float32Array.from(b)),
    inMin: data.inMin, inMax: data.inMax, labels: data.legend.slice() };
  const job = { ...rows_of(data), y: data.y, nVal: sp.nVal, batchSize: o.batchSize === undefined ? 32 : o.batchSize, learningRate: opt.learningRate, epochs,
    orders: o.orders || tm.epochOrders(sp.nTrain, epochs, seed + 1) };
  return { spec, job, onEpoch: typeof o.onEpoch === 'function' ? o.onEpoch : undefined };
}
function trained_handle(plan, r) {    // the model handle of a finished run `r` of the addon's train / trainGroup
  const h = { spec: Object.assign({}, plan.spec, { kernels: r.kernels, biases: r.biases }), natives: new Map(), released: false, history: [] };
  for (let e = 0; e < plan.job.epochs; e++) h.history.push({ loss: r.history[4 * e], acc: r.history[4 * e + 1], val_loss: r.history[4 * e + 2], val_acc: r.history[4 * e + 3] });
  h.labels = h.spec.labels.slice();
  loaded_models.add(h);
  return h;
}
// a run's rows for the addon's train: host rows, or the rows of a device DB by index (they stay on the device)
function rows_of(data) { return data.db ? { db: data.db.native, rows: data.rows32 } : { features: data.features }; }
function train_context() {
  const nat = addon();
  return { nat, ctx: contexts_for(nat, settings.devices ? settings.devices.slice() : [settings.device])[0] };
}
function trainModel(o) {
  let plan, t;
  try { plan = plan_train_model(o); t = train_context(); } catch (e) { return Promise.reject(e); }
  return t.nat.train(t.ctx, plan.spec, plan.job, plan.onEpoch).then((r) => trained_handle(plan, r));
}
// ---- the app's regression models for the ordinal labels V, A and D (ref src/neuralmodel.js:268-333 train_nn's ordinal branch, :410-585 predict_db_nn /
// predict_single; specification TR-2, include/wsa.h "Regression models").
// trainRegression(features: [[53 numbers]], values, {options, epochs, batchSize, seed, validationSplit, init, orders, onEpoch}) -> Promise of a model
// handle; `values` holds per row the label's value (null: unlabelled), `options` defaults to the app's nn_default_options_ords.  The handle carries
// `history` and spec.outMin / spec.outMax; saveModel / loadModel write and read its directory (dist/nnmodel/<db>/ords_<label>/).
// predictValues(handle, features: [[53 numbers]]) -> Float64Array, per row what ml5's predictMultiple gives as result[0].value.
// A regression handle is not a prediction model: setPredictionModel(s) need class probabilities, and trainModel keeps refusing a stack without softmax.
function plan_train_regression(features, values, o) {
  const tm = require('./trainmodel.js');
  const opt = Object.assign({}, tm.DEFAULT_OPTIONS_ORDS, o.options || {});
  const data = is_device_db(features) ? device_db_data(features, tm.selectOrdinal(values), values.length) : tm.prepareOrdinal(features, values);
  const st = tm.stackRegression(opt.layers, data.width), epochs = o.epochs === undefined ? 10 : o.epochs | 0, seed = o.seed | 0;
  const sp = tm.split(data.values.length, o.validationSplit);
  const init = o.init || tm.glorotInit(Array.from(st.units), seed);
  const spec = { units: st.units, activation: st.activation, kernels: init.kernels.map((k) => Float32Array.from(k)), biases: init.biases.map((b) => Float32Array.from(b)),
    inMin: data.inMin, inMax: data.inMax, labels: [], outMin: data.outMin, outMax: data.outMax };
  const job = { ...rows_of(data), values: data.values, outMin: data.outMin, outMax: data.outMax, nVal: sp.nVal, batchSize: o.batchSize === undefined ? 32 : o.batchSize,
    learningRate: opt.learningRate, epochs, orders: o.orders || tm.epochOrders(sp.nTrain, epochs, seed + 1) };
  return { spec, job, onEpoch: typeof o.onEpoch === 'function' ? o.onEpoch : undefined };
}
function trainRegression(features, values, o) {
  let plan, t;
  try { plan = plan_train_regression(features, values, o || {}); t = train_context(); } catch (e) { return Promise.reject(e); }
  return t.nat.train(t.ctx, plan.spec, plan.job, plan.onEpoch).then((r) => trained_handle(plan, r));
}
// ---- several models at once (K7g / specification TG-1, include/wsa.h "Training groups"): the app needs one model per DB and head, and at ml5's batch of 32
// an epoch is bound by its launches, so the jobs' trainers step in lock step, one launch per stage for all of them.
// trainModels(jobs) -> Promise of an array of model handles, in job order, identical to the handles of one-by-one calls.  A job is either the object
// trainModel takes or {regression: true, features, values, ...trainRegression's options}; onEpoch is per job.  A job with fewer epochs stops stepping;
// more than 32 jobs run as consecutive groups of 32.
const TRAIN_GROUP_MAX = 32;
function trainModels(jobs) {
  let plans, t;
  try {
    if (!Array.isArray(jobs)) throw 'trainModels(jobs): an array of trainModel objects and {regression: true, features, values, ...} objects';
    plans = jobs.map((o) => (o && o.regression ? plan_train_regression(o.features, o.values, o) : plan_train_model(o)));
    t = train_context();
  } catch (e) { return Promise.reject(e); }
  let chain = Promise.resolve([]);
  for (let first = 0; first < plans.length; first += TRAIN_GROUP_MAX) {
    const part = plans.slice(first, first + TRAIN_GROUP_MAX);
    chain = chain.then((done) => t.nat.trainGroup(t.ctx, part.map((p) => (p.onEpoch ? [p.spec, p.job, p.onEpoch] : [p.spec, p.job])))
      .then((rs) => done.concat(rs.map((r, i) => trained_handle(part[i], r)))));
  }
  return chain;
}
function predictValues(handle, features) {
  if (!loaded_models.has(handle) || handle.released) throw 'predictValues: the model handle was released (shutdown()) or is not one of loadModel / trainRegression';
  if (typeof handle.spec.outMin !== 'number' || typeof handle.spec.outMax !== 'number') throw 'predictValues: not a regression model (no output range)';
  if (!Array.isArray(features)) throw 'predictValues(handle, [[53 numbers]])';
  const W = handle.spec.units[0];       // 53, or the 264 / 23 of a model trained on level-11 / level-12 rows
  const x = new Float64Array(features.length * W);
  features.forEach((row, r) => {
    if (row.length !== W) throw 'predictValues: row ' + r + ' has ' + row.length + ' features; ' + W + ' expected';
    for (let k = 0; k < W; k++) x[r * W + k] = Number(row[k]);
  });
  const nat = addon();
  const ctx = contexts_for(nat, settings.devices ? settings.devices.slice() : [settings.device])[0];
  let m = handle.natives.get(ctx);
  if (!m) { m = nat.modelCreate(ctx, handle.spec); handle.natives.set(ctx, m); }
  return nat.regressRows(ctx, m, x, handle.spec.outMin, handle.spec.outMax);
}
// ---- predicting a labelled feature DB and the app's results table (ref src/neuralmodel.js:410-535 predict_db_nn, src/localstore.js:723-769
// update_pred_label, :498-627 shows_stats_table; specification DS-1 / K8, include/wsa.h "Predicting a labelled feature DB"): what replaces the app's
// Predict button and results panel.
// predictDB(featureDB, {db, type: 'cats'|'ords', label, model | modelDir, classLabels, ordinalLabels}) runs the model over EVERY sample of the DB
// (featuredb.js), fills the samples' `pred` pairs by update_pred_label's rule and returns the per-row predictions (labels or null / values);
// FeatureDB.to_json / to_csv then export the pred_<name> columns as for imported pairs.
// statsTable(featureDB, {db, classLabels, ordinalLabels}) -> {cats, ords, lines}: the table as data and the text the app prints (dbstats.js).
function dbstats_device() {
  const nat = addon();
  const ctx = contexts_for(nat, settings.devices ? settings.devices.slice() : [settings.device])[0];
  return {
    predict(handle, x, ords) {
      if (!loaded_models.has(handle) || handle.released) throw 'predictDB: the model handle was released (shutdown()) or is not one of loadModel / trainModel / trainRegression';
      let m = handle.natives.get(ctx);
      if (!m) { m = nat.modelCreate(ctx, handle.spec); handle.natives.set(ctx, m); }
      return ords ? nat.dbPredict(ctx, m, x, true, handle.spec.outMin, handle.spec.outMax) : nat.dbPredict(ctx, m, x, false);
    },
    table(col) { return nat.dbTable(ctx, col); },
    evaluate(spec, catHandles, ordHandles) {
      const native_of = (handle) => {
        if (!handle) return null;
        if (!loaded_models.has(handle) || handle.released) throw 'evaluateDB: the model handle was released (shutdown()) or is not one of loadModel / trainModel / trainRegression';
        let m = handle.natives.get(ctx);
        if (!m) { m = nat.modelCreate(ctx, handle.spec); handle.natives.set(ctx, m); }
        return m;
      };
      const natives_of = (h) => (Array.isArray(h) ? h.map(native_of) : native_of(h));          // an array: the folds' models of a head (CV-1)
      return nat.dbEval(ctx, Object.assign({}, spec, { catModels: catHandles.map(natives_of), ordModels: ordHandles.map(natives_of) }));
    },
  };
}
function predictDB(featureDB, o) {
  o = Object.assign({}, o || {});
  if (!o.model && o.modelDir) o.model = loadModel(o.modelDir);
  if (!o.model || !o.model.spec) throw "predictDB(featureDB, {db, type: 'cats'|'ords', label, model | modelDir, classLabels, ordinalLabels})";
  return require('./dbstats.js').predictDB(dbstats_device(), featureDB, o);
}
function statsTable(featureDB, o) { return require('./dbstats.js').statsTable(dbstats_device(), featureDB, o || {}); }
// evaluateDB(featureDB, {db, classLabels, ordinalLabels, models: {head name: model handle | model directory}, perFile}) -> {rows, files}: beyond the
// panel (specification EV-1 / K8e, include/wsa_eval.h, the addon's dbEval): DS-1's table, a confusion matrix per categorical head (recall, precision,
// UAR) and CCC / Pearson per ordinal head, per row and per file — a file's class from the app's own fold over the file's callbacks, its value the
// running value; the same structure as webspeechanalyzer_amd.dbstats.evaluate, as plain JSON-able data with the text lines.
function evaluateDB(featureDB, o) {
  o = Object.assign({}, o || {});
  const models = {};
  for (const name of Object.keys(o.models || {})) models[name] = typeof o.models[name] === 'string' ? loadModel(o.models[name]) : o.models[name];
  o.models = models;
  return require('./dbstats.js').evaluateDB(dbstats_device(), featureDB, o);
}
// crossValidate(featureDB, {db, classLabels, ordinalLabels, heads: [names], k, groupOf, foldOfFile, options, epochs, batchSize, validationSplit, seed,
// perFile, keepModels}) -> Promise of evaluateDB's {rows, files} plus folds, foldOfRow, foldOfFile (and models with keepModels): K-fold
// cross-validation with a file's rows on one side of every split (specification CV-1, js/crossval.js; webspeechanalyzer_amd.crossval in Python).
function crossValidate(featureDB, o) {
  try { return require('./crossval.js').crossValidate({ trainModels, evaluate: (db, e) => require('./dbstats.js').evaluateDB(dbstats_device(), db, e) }, featureDB, o || {}); }
  catch (e) { return Promise.reject(e); }
}
// ---- the app's ml5 KNN classifier (ref src/neuralmodel.js:729-837 train_knn; specification KN-1 / K9, include/wsa.h "KNN classifier"; js/knn.js).
// KNNClassifier(width, capacity) -> ml5.KNNClassifier()'s addExample / classify / getCountByLabel on the device (classify is synchronous and
//   returns ml5's result object; addExamples / classifyMultiple take many rows at once);
// trainKnn(featureDB, {db, label, classes, k}) -> {knn, samples, correct, all}: train_knn's procedure over a feature DB (featuredb.js);
// predictKnn(knn, [[numbers]], k) -> ml5's result per row.  knn.release() frees the device store (shutdown() frees it with its context).
function knn_device() {
  const nat = addon();
  const ctx = contexts_for(nat, settings.devices ? settings.devices.slice() : [settings.device])[0];
  return {
    create: (width, classes, capacity) => nat.knnCreate(ctx, width, classes, capacity),
    add: (store, x, cls) => nat.knnAdd(store, x, cls),
    classify: (store, x, k) => nat.knnClassify(store, x, k),
    batch: (store, k) => nat.batchKnn(ctx, store, k),
    destroy: (store) => nat.knnDestroy(store),
  };
}
function KNNClassifier(width, capacity) { return new (require('./knn.js').KnnClassifier)(knn_device(), width === undefined ? 53 : width, capacity); }
function trainKnn(featureDB, o) { return require('./knn.js').trainKnn(knn_device(), featureDB, o); }
function predictKnn(knn, rows, k) {
  if (!knn || typeof knn.classifyMultiple !== 'function' || !Array.isArray(rows)) throw 'predictKnn(knn, [[numbers]], k)';
  return knn.classifyMultiple(rows, k === undefined ? 10 : k);
}
// setPredictionKnn(knn | null, k, on_prediction): as setPredictionModel with a KNNClassifier of 53-feature rows in the model's place.  Every level-13
// LaunchBatch / LaunchBatches launch and every StreamOpen set opened from here on classifies its syllables with the store's k nearest rows (K9 / K9s)
// and folds them as the app folds a network's result (specification KN-2: votes / k per label, ties in class order), calling
//     on_prediction(si, [label, confidence], clip_or_stream_index, per_syllable)
// in setPredictionModel's shape; `meters` is one {label: Label_conf_all} per clip / stream.  The rows are those the classifier holds when a
// launch starts or a stream set opens (each context gets its own device copy of them).  setPredictionKnn and setPredictionModel(s) replace each other.
const knn_natives = new Map();          // context -> {knn, n, store}: the device copy of a prediction KNN's rows on that context
function setPredictionKnn(knn, k, on_prediction) {
  if (knn === null || knn === undefined) { prediction = null; return; }
  if (typeof knn !== 'object' || typeof knn.classifyMultiple !== 'function' || !Array.isArray(knn.labels)) throw 'setPredictionKnn(knn | null, k, on_prediction): knn is a KNNClassifier';
  if (knn.width !== 53) throw 'setPredictionKnn: the store holds rows of ' + knn.width + ' features; live prediction folds the 53-feature syllable rows of output_level 13';
  if (!Number.isInteger(k) || k < 1 || k > 64) throw 'setPredictionKnn: k must be 1 .. 64, got ' + String(k);
  if (!knn.store) throw 'setPredictionKnn: the KNN store was released';
  if (!knn.labels.length) throw 'setPredictionKnn: There is no example in any class';
  if (typeof on_prediction !== 'function') throw 'setPredictionKnn(knn | null, k, on_prediction)';
  prediction = { knn, k, on_prediction, get model() { return { labels: knn.names }; } };
}
function knn_store_on(nat, ctx, knn) {   // the prediction KNN's rows as a store on one context (made at its first use there, again when rows were added)
  if (!knn.store) throw 'the prediction KNN store was released';
  const e = knn_natives.get(ctx), n = knn.labels.length;
  if (e && e.knn === knn && e.n === n) return e.store;
  if (e) { knn_natives.delete(ctx); nat.knnDestroy(e.store); }
  const K = require('./knn.js');
  const store = nat.knnCreate(ctx, 53, K.MAX_CLASSES, n);
  nat.knnAdd(store, K.pack(knn.rows, 53, 'KNN'), knn.index);
  knn_natives.set(ctx, { knn, n, store });
  return store;
}
// K9 + KN-2 over the rows of the batch a context has just finished: the tables predict_after and meters_of read, under a model's names
function knn_fold_into(nat, ctx, res, pred) {
  const t = nat.batchKnn(ctx, knn_store_on(nat, ctx, pred.knn), pred.k), f = nat.batchKnnFold(ctx);
  res.prob = t.conf; res.nClasses = t.nClasses; res.cb = f.cb; res.cbLabel = f.cbLabel; res.cbConf = f.cbConf; res.clipConf = f.clipConf;
}
// setPredictionValues(handles | null, on_values): 1 .. 8 regression handles (loadModel of an ords_<label> directory, or trainRegression) — the app's V, A and D
// models — predicted in one grouped launch and folded per callback by specification RG-1 (DESIGN.md §3; ours: the reference wires `?type=ords` up, ref
// src/index.js:892-893, and its fold then sums fields a regression result does not have, ref src/prediction.js:96-101).  Every level-13 LaunchBatch /
// LaunchBatches launch and every StreamOpen set opened from here on calls, on the JS thread and in callback order, right after each segment's callback
// (and its on_prediction, if a prediction model is set too),
//     on_values(si, values[H], clip_or_stream_index, {weights, per_syllable, running})
// values[h] = the callback's sqrt(duration)-weighted mean of head h's per-syllable values (NaN: no usable row), weights[h] the sum of the weights,
// per_syllable[q][h] the rows' own values, running[h] the running weighted mean of the clip (or of the stream since its START) after this callback.
// A skipped callback (durations that sum to 0) gets no call, as on_prediction does not.  Independent of setPredictionModel, setPredictionModels and
// setPredictionKnn: it neither replaces them nor is replaced by them.
let value_prediction = null;
function setPredictionValues(handles, on_values) {
  if (handles === null || handles === undefined) { value_prediction = null; return; }
  if (!Array.isArray(handles) || handles.length < 1 || handles.length > 8) throw 'setPredictionValues([handles] | null, on_values): 1 .. 8 regression model handles';
  for (const h of handles) if (!loaded_models.has(h) || h.released) throw 'setPredictionValues: a model handle was released (shutdown()) or is not one of loadModel / trainRegression';
  for (const h of handles) if (typeof h.spec.outMin !== 'number') throw 'setPredictionValues: a classifier has no value to fold; setPredictionModel takes it';
  for (const h of handles) if (h.spec.units[0] !== 53) throw 'setPredictionValues: a model takes ' + h.spec.units[0] + ' inputs; live prediction folds the 53-feature syllable rows of output_level 13';
  if (typeof on_values !== 'function') throw 'setPredictionValues([handles] | null, on_values)';
  value_prediction = { models: handles.slice(), on_values };
}
// the native models and ranges of the value heads on one context (a model is created at its first use there)
function value_heads_on(nat, ctx, vp) {
  const models = vp.models.map((h) => {
    if (h.released) throw 'a value model was released (shutdown())';
    let m = h.natives.get(ctx);
    if (!m) { m = nat.modelCreate(ctx, h.spec); h.natives.set(ctx, m); }
    return m;
  });
  return [models, Float64Array.from(vp.models, (h) => h.spec.outMin), Float64Array.from(vp.models, (h) => h.spec.outMax)];
}
// the grouped launch + RG-1 over the rows of the batch a context has just finished
function values_fold_into(nat, ctx, res, vp) {
  res.reg = nat.batchRegressGroup(ctx, ...value_heads_on(nat, ctx, vp));
}
// RG-1's running sums per unit (clip / stream), kept here by the specification's own rule from the device's per-row values, so that the running value
// exists after EVERY callback (the device hands out each unit's last state); JavaScript's doubles round as the device's do, so the last one is the device's
function values_after(G, meta, r, si, unit, vp, accs) {
  if (!G.cbIndex) { G.cbIndex = new Map(); for (let k = 0; k < G.cb.length / 4; k++) G.cbIndex.set(G.cb[k * 4 + 2], k); }
  const k = G.cbIndex.get(r);
  if (k === undefined) return;
  const H = G.nHeads, K = G.cb.length / 4, R = G.value.length / H, n = G.cb[k * 4 + 3], step = settings.window_step / 1e3;
  const d = Array.from({ length: n }, (_, q) => parseFloat(((meta[(r + q) * 8 + 3] + 1) * step).toFixed(3)));
  let seg_weight = 0;
  for (const x of d) seg_weight += x;
  if (!(seg_weight > 0)) return;                                 // skipped: no call, the running sums untouched
  if (!accs.get(unit)) accs.set(unit, { A: new Array(H).fill(0), B: new Array(H).fill(0) });
  const acc = accs.get(unit);
  const per = Array.from({ length: n }, (_, q) => Array.from({ length: H }, (_, h) => G.value[h * R + r + q]));
  for (let h = 0; h < H; h++)
    for (let q = 0; q < n; q++) {
      const v = per[q][h], w = Math.sqrt(d[q]);
      if (!Number.isFinite(v)) continue;
      const t = v * w;
      acc.A[h] += t; acc.B[h] += w;
    }
  vp.on_values(si, Array.from({ length: H }, (_, h) => G.cbValue[h * K + k]), unit,
    { weights: Array.from({ length: H }, (_, h) => G.cbWeight[h * K + k]), per_syllable: per, running: acc.A.map((a, h) => (acc.B[h] !== 0 ? a / acc.B[h] : NaN)) });
}
// clip c's {sum, weight, value}, one entry per head, from a batch's RG-1 tables
function clip_values_of(G, c) {
  const H = G.nHeads, N = G.clipValue.length / H, at = (t) => Array.from({ length: H }, (_, h) => t[h * N + c]);
  return { sum: at(G.clipSum), weight: at(G.clipWeight), value: at(G.clipValue) };
}
function saveModel(handle, dir) {
  if (!handle || !handle.spec) throw 'saveModel(handle, dir)';
  require('./trainmodel.js').saveModelFiles(handle.spec, dir);
}
function setPredictionModel(handle, on_prediction) {
  if (handle === null || handle === undefined) { prediction = null; return; }
  if (!loaded_models.has(handle) || handle.released) throw 'setPredictionModel: the model handle was released (shutdown()) or is not one of loadModel';
  if (typeof handle.spec.outMin === 'number') throw 'setPredictionModel: a regression model has no class probabilities to fold; predictValues gives its values';
  if (handle.spec.units[0] !== 53) throw 'setPredictionModel: the model takes ' + handle.spec.units[0] + ' inputs; live prediction folds the 53-feature syllable rows of output_level 13';
  if (typeof on_prediction !== 'function') throw 'setPredictionModel(handle, on_prediction)';
  prediction = { model: handle, on_prediction };
}
function setPredictionModels(handles, on_prediction) {
  if (handles === null || handles === undefined) { prediction = null; return; }
  if (!Array.isArray(handles) || handles.length < 1 || handles.length > 8) throw 'setPredictionModels([handles], on_prediction): 1 .. 8 model handles';
  for (const h of handles) if (!loaded_models.has(h) || h.released) throw 'setPredictionModels: a model handle was released (shutdown()) or is not one of loadModel';
  for (const h of handles) if (typeof h.spec.outMin === 'number') throw 'setPredictionModels: a regression model has no class probabilities to fold; predictValues gives its values';
  for (const h of handles) if (h.spec.units[0] !== 53) throw 'setPredictionModels: a model takes ' + h.spec.units[0] + ' inputs; live prediction folds the 53-feature syllable rows of output_level 13';
  if (typeof on_prediction !== 'function') throw 'setPredictionModels([handles], on_prediction)';
  // the carried min_entropy_db is an index into the list: the same list keeps it (the reference's available_DBs never changes), another list starts anew
  const same = prediction && prediction.models && prediction.models.length === handles.length && prediction.models.every((h, i) => h === handles[i]);
  prediction = { models: handles.slice(), on_prediction, state: same ? prediction.state : { min_db: null } };
}
function release_models() {           // shutdown(): the native models go with their contexts; the handles are refused from here on
  for (const h of loaded_models) { h.released = true; h.natives.clear(); }
  loaded_models.clear();
  knn_natives.clear();                  // (the stores went with their contexts)
  prediction = null; value_prediction = null;
}
function model_on(nat, ctx) {         // the native model of the prediction model on one context (created at its first use there)
  if (!prediction || prediction.knn || settings.output_level !== 13) return undefined;
  const one = (h) => {
    if (h.released) throw 'the prediction model was released (shutdown())';
    let m = h.natives.get(ctx);
    if (!m) { m = nat.modelCreate(ctx, h.spec); h.natives.set(ctx, m); }
    return m;
  };
  return prediction.models ? prediction.models.map(one) : one(prediction.model);      // (an array: the addon classifies with the ensemble of them)
}
function forget_natives(pred, ctx) {
  if (pred.knn) { knn_natives.delete(ctx); return; }
  for (const h of pred.models || [pred.model]) h.natives.delete(ctx);
}
const has_cb = (res) => !!(res.cb || (res.ens && res.ens.cb));
// per clip: Label_conf_all as {label: sum} in legend order (labels never added: 0)
function meters_of(res, clip, labels) {
  const C = res.nClasses, o = {};
  for (let c = 0; c < C && c < labels.length; c++) o[labels[c]] = res.clipConf[clip * C + c];      // (a KNN store has 64 classes, its classifier fewer labels)
  return o;
}
// the prediction of the level-13 callback whose first row is r (res.cb lists them in row order)
function predict_after(res, r, si, clip, pred) {
  if (pred.models) { predict_after_ensemble(res, r, si, clip, pred); return; }
  if (!res.cbIndex) { res.cbIndex = new Map(); for (let k = 0; k < res.cb.length / 4; k++) res.cbIndex.set(res.cb[k * 4 + 2], k); }
  const k = res.cbIndex.get(r);
  if (k === undefined || res.cbLabel[k] === -2) return;
  const labels = pred.model.labels, C = res.nClasses, n = res.cb[k * 4 + 3];
  const sorted = (q) => {
    const e = [];
    for (let c = 0; c < C && c < labels.length; c++) e.push({ [labels[c]]: res.prob[q * C + c], label: labels[c], confidence: res.prob[q * C + c] });
    return e.sort((a, b) => b.confidence - a.confidence);             // ml5 classifyInternal (a stable sort: ties keep legend order)
  };
  const per = n === 1 ? sorted(r) : Array.from({ length: n }, (_, q) => sorted(r + q));
  const lab = res.cbLabel[k] >= 0 ? labels[res.cbLabel[k]] : null;
  pred.on_prediction(si, [lab, res.cbConf[k]], clip, per);
}

// the share of each label in an accumulator's sum, keys and additions in Object.keys order (ref prediction.js:180-191)
function shares_of(acc) {
  const keys = Object.keys(acc), o = {};
  let sum = 0;
  for (const k of keys) sum += acc[k];
  for (const k of keys) o[k] = acc[k] / sum;
  return o;
}
// with an ensemble: res.ens holds the device's tables; the accumulators behind the meters are kept here per launch unit (clip / stream), by the
// reference's own rule (ref prediction.js:91-115), so that the gauges exist after EVERY callback (the device hands out only each unit's last state)
function predict_after_ensemble(res, r, si, unit, pred) {
  const E = res.ens;
  if (!E.cbIndex) { E.cbIndex = new Map(); for (let k = 0; k < E.cb.length / 4; k++) E.cbIndex.set(E.cb[k * 4 + 2], k); }
  const k = E.cbIndex.get(r);
  if (k === undefined || E.cbDb[k] === -2) return;
  const n = E.cb[k * 4 + 3], step = settings.window_step / 1e3;
  const accs_of = pred.accs || (res.ensAccs = res.ensAccs || new Map());
  if (!accs_of.get(unit)) accs_of.set(unit, pred.models.map(() => ({})));
  const accs = accs_of.get(unit);
  const per_db = pred.models.map((h, d) => {
    const labels = h.labels, C = E.nClasses[d], prob = E.prob[d];
    const sorted = (q) => {
      const e = [];
      for (let c = 0; c < C; c++) e.push({ [labels[c]]: prob[q * C + c], label: labels[c], confidence: prob[q * C + c] });
      return e.sort((a, b) => b.confidence - a.confidence);
    };
    const per = n === 1 ? sorted(r) : Array.from({ length: n }, (_, q) => sorted(r + q));
    for (let q = 0; q < n; q++) {
      const w = Math.sqrt(parseFloat(((res.meta[(r + q) * 8 + 3] + 1) * step).toFixed(3)));
      for (const e of (n === 1 ? [per[0]] : per[q])) {
        const wc = e.confidence * w;
        if (!accs[d][e.label]) accs[d][e.label] = wc; else accs[d][e.label] += wc;
      }
    }
    return { label: E.cbLabel[d][k] >= 0 ? labels[E.cbLabel[d][k]] : null, confidence: E.cbConf[d][k], per_syllable: per };
  });
  const db = E.cbDb[k];
  if (E.cbMinDb[k] >= 0) pred.state.min_db = E.cbMinDb[k];
  const m = pred.state.min_db;
  const fresh = E.cbMinDb[k] >= 0;                       // else: a DB carried from an earlier launch, whose accumulator of this one has nothing above 0
  const meters = m === null ? {} : shares_of(accs[m] || {});
  const entropy = fresh ? E.cbEntropy[k] : NaN;
  pred.on_prediction(si, [db >= 0 ? pred.models[db].labels[E.cbTopLabel[k]] : null, E.cbTopConf[k]], unit,
    { db: db >= 0 ? db : null, per_db, min_entropy_db: m, entropy, meters });
}
// (a clip without a callback of its own says nothing: the carried DB stays)
// the resolved result's meters of one clip / stream: those of its own min_entropy_db, from the accumulators kept while dispatching (else the
// device's sums, added in legend order)
function ensemble_meters_of(res, unit, pred, accs_of) {
  const E = res.ens, m = E.minDb[unit];
  if (m < 0) return {};
  const kept = accs_of && accs_of.get(unit);
  if (kept) return shares_of(kept[m]);
  const C = E.nClasses[m], acc = {};
  pred.models[m].labels.forEach((l, c) => { if (E.conf[m][unit * C + c] !== 0) acc[l] = E.conf[m][unit * C + c]; });
  return shares_of(acc);
}

// rows of one clip -> the reference's callback sequence (ref dispatcher P() @B28869)
function dispatch(res, clip, callback, label, pred = null, clip_index = clip, vp = null) {
  const level = settings.output_level, step = settings.window_step / 1e3;
  const a = res.rowOff[clip], b = res.rowOff[clip + 1];
  const feat = (r) => Array.from(res.feat.subarray(r * 53, r * 53 + 53));
  if (level === 5) {
    for (let r = a; r < b; r++) {
      if (stop_requested) return;
      const m = res.meta.subarray(r * 8, r * 8 + 8);
      callback(m[1], label, [m[2] * step, (m[3] + 1) * step], feat(r));                       // ref @B29622, @B31504
    }
  } else if (level === 13 || level === 12) {
    const nf = level === 12 ? 23 : 53;          // level 12: the polynomial coefficients of make_coeffs (ref @B34150)
    let r = a;
    while (r < b) {
      if (stop_requested) return;
      const si = res.meta[r * 8 + 1];
      const times = [], feats = [];
      let cut = false;
      while (r < b && res.meta[r * 8 + 1] === si) {
        const m = res.meta.subarray(r * 8, r * 8 + 8);
        times.push([(m[2] * step).toFixed(3), ((m[3] + 1) * step).toFixed(3)]);              // ref @B31114
        // level 12: a syllable on which numeric.uncmin threw ends the segment's list (ref make_coeffs' try / catch @B34150)
        if (nf === 23 && res.feat[r * 53 + 23] !== 0) cut = true;
        if (!cut) feats.push(nf === 53 ? feat(r) : Array.from(res.feat.subarray(r * 53, r * 53 + nf)));
        r++;
      }
      if (feats.length > 0) {
        if (callback) callback(si, label, times, feats);                                      // ref @B29138 (`p[e].length>0`)
        if (pred && has_cb(res) && level === 13) predict_after(res, r - times.length, si, clip_index, pred);       // ref src/index.js:56 -> prediction.js:70
        if (vp && res.reg && res.reg.cb && level === 13) values_after(res.reg, res.meta, r - times.length, si, clip_index, vp, res.regAccs || (res.regAccs = new Map()));
      }
    }
  } else if (level === 11) {
    // utterance features: after every result the 264 histogram bins over everything so far, callback index 0 (ref @B28869)
    for (let k = res.uttOff[clip]; k < res.uttOff[clip + 1]; k++) {
      if (stop_requested) return;
      const m = res.uttMeta.subarray(k * 4, k * 4 + 4);
      callback(0, label, [m[2] * step, (m[3] + 1) * step], Array.from(res.uttFeat.subarray(k * 264, k * 264 + 264)));     // ref Y() @B31330
    }
  } else if (level === 4 || level === 10) {
    // the straightened frames themselves: Float32Array(9) per frame = 3 x (bin, band energy, width), ref @B35074
    const base = res.frameOff[clip];
    const frames = (m) => { const o = [], a0 = (base + m[6]) * 9; for (let d = 0; d < m[7]; d++) o.push(res.formants.slice(a0 + 9 * d, a0 + 9 * d + 9)); return o; };
    let r = a;
    while (r < b) {
      if (stop_requested) return;
      const m = res.meta.subarray(r * 8, r * 8 + 8);
      if (level === 4) { callback(m[1], label, [m[2] * step, (m[3] + 1) * step], frames(m)); r++; continue; }          // ref @B28124
      const si = m[1], times = [], syl = [];
      while (r < b && res.meta[r * 8 + 1] === si) {
        const q = res.meta.subarray(r * 8, r * 8 + 8);
        times.push([(q[2] * step).toFixed(3), ((q[3] + 1) * step).toFixed(3)]);
        syl.push(frames(q)); r++;
      }
      callback(si, label, times, syl);                                                                                  // ref @B27713
    }
  } else if (level === 3) {
    // the ranked raw tracks of every segment, three-argument callback (ref @B28273 `s.push(i)`, @B30132 `b(e, label, s[e])`)
    for (let k = res.segOff[clip]; k < res.segOff[clip + 1]; k++) {
      if (stop_requested) return;
      const tr = tracks_of_segment(res, k);
      if (tr.length > 0) callback(k - res.segOff[clip], label, tr);
    }
  } else {
    throw 'output_level ' + level + ' is not available through this build (3, 4, 5, 10, 11, 12 and 13 are)';
  }
}

// level 3: the 18-field track records of accumulate_fm (ref @B35952; field map SURVEY.md App. A) rebuilt from the per-point
// entries libwsa hands out (include/wsa.h wsa_batch_copy_tracks): every other field is a function of the six point arrays
function tracks_of_segment(res, k) {
  const p0 = res.trackOff[2 * k], p1 = res.trackOff[2 * k + 2], r0 = res.trackOff[2 * k + 1], r1 = res.trackOff[2 * k + 3];
  const per = new Map();
  const f64 = new Float64Array(1), i32 = new Int32Array(f64.buffer);
  for (let q = p0; q < p1; q++) {
    const t = res.trackPoints[8 * q];
    if (!per.has(t)) per.set(t, []);
    per.get(t).push(q);
  }
  const out = [];
  for (let r = r0; r < r1; r++) {
    const P = per.get(res.trackRanked[r]);
    const frames = [], starts = [], ends = [], bins = [], amps = [], energies = [];
    let sE = 0, sEb = 0, sW = 0;
    for (const q of P) {
      const w = res.trackPoints.subarray(8 * q, 8 * q + 8);
      i32[0] = w[2]; i32[1] = w[3];
      const be = f64[0], bin = w[1] & 0xff;
      frames.push(w[6]); starts.push(w[4]); ends.push(w[7]); bins.push(bin); amps.push(w[5] >>> 0); energies.push(be);
      sE += be; sEb += be * bin; sW += w[7] - w[4] + 1;                                      // ref @B36776 [13] [15] [17]
    }
    const h = P.length - 1, pb = bins[h];                                                   // velocity of the last update, ref @B36624
    const vel = h === 0 ? 0 : (h === 1 ? pb - bins[0] : (h === 2 ? ((pb - bins[1]) + (bins[0] - bins[1])) / 2
      : ((pb - bins[h - 1]) + (bins[h - 2] - bins[h - 1]) + (bins[h - 3] - bins[h - 2])) / 3));
    out.push([starts[h], ends[h], frames[h], frames[h], vel, pb, amps[h], frames, starts, ends, bins, amps, energies, sE, P.length, sEb, 0, sW]);
  }
  return out;
}

// what processBatch takes as the clips' rate: the number when they share one, else a Float64Array with one rate per clip
function rates_of(clips) {
  return clips.every((c) => c.sampleRate === clips[0].sampleRate) ? clips[0].sampleRate : Float64Array.from(clips, (c) => c.sampleRate);
}

// contiguous block partition of n clips over k shards (the first n % k shards take one more)
function shard_ranges(n, k) {
  const out = [], q = Math.floor(n / k), r = n % k;
  for (let i = 0, a = 0; i < k; i++) { const b = a + q + (i < r ? 1 : 0); out.push([a, b]); a = b; }
  return out;
}

async function run(clips, callback, labels_of, test_play) {
  const nat = addon();
  if (playing) throw 'Error: Already playing';                                               // ref @B4554
  playing = true; stop_requested = false; labels_per_segment = [];
  try {
    // one geometry per launch: without a conversion in front the clips must share a rate; with resample_to every clip is converted from its own
    // (what the app's folder loop gets from decodeAudioData, ref src/index.js:277-296) and a clip already at resample_to passes unfiltered
    // a collecting DB and several contexts do not go together: said before the contexts of the new device list replace the DB's
    if (collect_db && several_devices()) throw several_devices_message();
    const rates = new Set(clips.map((c) => c.sampleRate));
    if (rates.size !== 1 && !(settings.resample_to > 0)) throw 'All clips of one launch must share a sample rate';
    const fs = clips[0].sampleRate;
    const fs_an = settings.resample_to > 0 ? settings.resample_to : fs;         // the rate the analysis runs at (K0 converts in front, spec RS-1)
    // clips are independent launches (SURVEY.md 8e): shard them contiguously over the configured devices, one context each; every
    // shard is one napi_async_work, i.e. its own worker thread (contexts are not thread-safe, distinct contexts are)
    const devs = settings.devices && clips.length > 1 ? settings.devices.slice(0, clips.length) : [settings.device];
    const shards = shard_ranges(clips.length, devs.length);
    const ctxs = contexts_for(nat, devs);
    const g = nat.geometry(ctxs[0], fs_an);
    const bands = settings.spec_type === 1 ? settings.N_mel_bins : settings.N_fft_bins;
    if (g.bands !== bands) throw 'Bins count mismatch: ' + g.bands + ', ' + bands;              // ref @B8568 check
    // (the clips travel as they are, whatever they hold: submit_clips)
    // the feature rows of all shards in one piece: they stay on their devices, one grouped RCCL send / receive over xGMI moves them to the first
    // device (include/wsa.h wsa_gather_rows) and ONE copy brings them to the host; a shard's small tables (segments, offsets) come with its own job
    const files = collect_db ? clips.map((_, c) => (labels_of(c) || [])[0]) : null;
    const cdb = collect_db ? collect_check(ctxs[0], files) : null;
    const gather = (settings.output_level === 5 || settings.output_level === 13) && (settings.gather === null ? devs.length > 1 && new Set(devs).size === devs.length : settings.gather);      // (a rank is a GPU: contexts that share a device are not gathered)
    const pred = prediction && settings.output_level === 13 ? prediction : null;
    const models = ctxs.map((c) => (pred ? model_on(nat, c) : undefined));
    const job = ([a, b], i) => {
      const part = clips.slice(a, b);
      const extra = pred && !pred.knn ? [models[i]] : [];        // (no model: the addon is called exactly as before; a KNN store classifies behind the job)
      const fs_i = rates_of(part);                               // (a shard whose clips share a rate: the number, as before)
      return submit_clips(nat, ctxs[i], part, fs_i, fs_an, gather, extra);
    };
    // every shard runs to its end before anything else happens (a context with work in flight must not be touched), then the
    // first failure, if any, is what the launch rejects with
    const settled = await Promise.allSettled(shards.map(job));
    const failed = settled.find((r) => r.status === 'rejected');
    if (failed) { drop_contexts(nat); throw failed.reason; }
    const results = settled.map((r) => r.value);
    if (gather) {
      let all;
      try { all = await nat.gatherRows(ctxs); } catch (e) { drop_contexts(nat); throw e; }
      for (let i = 0, off = 0; i < results.length; i++) {        // a shard's rows = its slice of the gathered tables (views, no copy)
        const k = all.rowsPerRank[i];
        results[i].meta = all.meta.subarray(off * 8, (off + k) * 8); results[i].feat = all.feat.subarray(off * 53, (off + k) * 53);
        off += k;
      }
    }
    if (cdb && results.length !== 1) throw 'setCollectDB: the launch ran as ' + results.length + ' shards; a device DB takes the rows of one context';      // (collect_check refuses it before anything runs)
    if (cdb) collect_append(nat, ctxs[0], cdb, results[0], files);       // (one shard; a refusal — the DB is full — rejects the launch, the DB unchanged)
    if (pred && pred.knn) {
      try { results.forEach((res, i) => knn_fold_into(nat, ctxs[i], res, pred)); } catch (e) { drop_contexts(nat); throw e; }
    }
    const vp = value_prediction && settings.output_level === 13 ? value_prediction : null;
    if (vp) {
      try { results.forEach((res, i) => values_fold_into(nat, ctxs[i], res, vp)); } catch (e) { drop_contexts(nat); throw e; }
    }
    // StopAudioNodes while the work was in flight: the reference tears the nodes down at the next frame and resolves (ref @B8851) —
    // nothing is dispatched any more, the launch still resolves
    if (!test_play && (callback || pred || vp)) {                                             // ref @B24762: silent when test_play
      for (let i = 0; i < shards.length && !stop_requested; i++)
        for (let c = shards[i][0]; c < shards[i][1] && !stop_requested; c++) dispatch(results[i], c - shards[i][0], callback, labels_of(c), pred, c, vp);
    }
    // per clip: the device's running sums and value of every head (not `values`: results is an Array)
    if (vp) results.head_values = [].concat(...shards.map(([a, b], i) => Array.from({ length: b - a }, (_, c) => clip_values_of(results[i].reg, c))));
    if (pred && pred.models) {
      // (dispatch numbers the clips of all shards 0 .. n - 1, a shard's tables its own from 0)
      results.meters = [].concat(...shards.map(([a, b], i) => Array.from({ length: b - a }, (_, c) =>
        ensemble_meters_of(results[i], c, pred, results[i].ensAccs && new Map([[c, results[i].ensAccs.get(a + c)]])))));
      results.min_entropy_db = [].concat(...shards.map(([a, b], i) => Array.from(results[i].ens.minDb.subarray(0, b - a), (v) => (v >= 0 ? v : null))));
      results.shown_min_entropy_db = pred.state.min_db;     // what the app's gauges still show: the last DB any launch had (the reference's global)
    } else if (pred) results.meters = [].concat(...shards.map(([a, b], i) => Array.from({ length: b - a }, (_, c) => meters_of(results[i], c, pred.model.labels))));
    return results;
  } finally {
    playing = false;
  }
}

// ---- the feature DB that stays on the GPU (specification FD-1, include/wsa.h "A feature DB that stays on the device"; the addon's featdb*).
// createDeviceDB(level, capacity) -> a DB of `capacity` rows of the level's vectors (5 / 13: 53 numbers, 11: 264, 12: 23) on the configured device.
// setCollectDB(db | null): every LaunchBatch / LaunchBatches launch from then on appends its run to `db` by the app's storing rules (ref src/index.js:35-100)
// before the batch's tables are reused — the vectors never leave the device for it; callbacks are delivered exactly as without it.  The file name of a
// clip is labels[clip][0], as the collector of js/featuredb.js takes it; a file the DB already holds is refused before anything runs (the app skips
// it, src/index.js:277).  A device DB lives on ONE device, in one context: with more than one entry in `devices` (also [0, 0]: every entry is a context
// of its own that takes a shard of the launch) setCollectDB is refused, and so is a launch while a DB collects.  While a DB collects, LaunchBatches
// runs its batches one after the other on the DB's context instead of pipelining them through two.
// db.records: per stored row {file, part, time, truth, guess}; db.count(); db.toFeatureDB(db_id) -> an ordinary FeatureDB (one copy of the vectors to the
// host); db.close().  trainModel({db, labels, classes, ...}) and trainRegression(db, values, ...) take the DB in place of `features` (labels / values: one
// per stored row): the ranges are taken on the device and the trainer reads the rows where they are.  predictDB, statsTable and the KNN functions take host rows.
const LEVEL_WIDTH = { 5: 53, 13: 53, 11: 264, 12: 23 };
let collect_db = null;
function is_device_db(v) { return Boolean(v) && typeof v === 'object' && v.native !== undefined && typeof v.toFeatureDB === 'function'; }
function live_device_db(db, who) {
  if (!is_device_db(db)) throw who + ': not a device DB (createDeviceDB)';
  if (db.released) throw who + ': the device DB was closed';
  if (!ctx_cache.ctxs.includes(db.ctx)) throw who + ': the device DB was created under other settings (its context is gone)';
  return db;
}
function createDeviceDB(level, capacity) {
  const width = LEVEL_WIDTH[level];
  if (!width) throw 'createDeviceDB: output_level ' + level + ' stores no feature vectors (5, 11, 12 and 13 do)';
  const t = train_context();
  const db = { level, width, capacity, ctx: t.ctx, native: t.nat.featdbCreate(t.ctx, width, capacity), records: [], files: new Set(), released: false };
  db.count = () => addon().featdbCount(live_device_db(db, 'count').native);
  db.toFeatureDB = (db_id) => {
    const { FeatureDB } = require('./featuredb.js');
    const rows = addon().featdbCopyRows(live_device_db(db, 'toFeatureDB').native), out = new FeatureDB();
    db.records.forEach((r, i) => {
      out.put(level, db_id, r.file, r.part, r.time, Array.from(rows.subarray(i * width, (i + 1) * width)));
      if (r.truth || r.guess) { const smp = out.table(db_id, false).get(FeatureDB.key(db_id, r.file, r.part)); smp.truth = r.truth || null; smp.guess = r.guess || null; }
    });
    return out;
  };
  db.close = () => { if (!db.released) { if (collect_db === db) collect_db = null; if (ctx_cache.ctxs.includes(db.ctx)) addon().featdbDestroy(db.native); db.released = true; } };
  return db;
}
// more than one entry in `devices` shards a launch over as many contexts, also where the entries name one GPU twice: a DB belongs to ONE context
function several_devices() { return Boolean(settings.devices) && settings.devices.length > 1; }
function several_devices_message() {
  return 'setCollectDB: a device DB lives on one device, in one context; `devices` has ' + settings.devices.length + ' entries, one context each (configure({devices: null}))';
}
function setCollectDB(db) {
  if (db === null || db === undefined) { collect_db = null; return; }
  if (several_devices()) throw several_devices_message();
  collect_db = live_device_db(db, 'setCollectDB');
}
// before a collecting launch: the DB fits the launch, and none of its files is held already
function collect_check(ctx, files) {
  const db = live_device_db(collect_db, 'setCollectDB');
  if (several_devices()) throw several_devices_message();
  if (db.ctx !== ctx) throw 'setCollectDB: the launch runs on another context than the device DB';
  if (db.level !== settings.output_level) throw 'setCollectDB: the DB holds the vectors of output_level ' + db.level + ', the launch runs at ' + settings.output_level;
  files.forEach((f, i) => { if (db.files.has(f) || files.indexOf(f) < i) throw 'setCollectDB: the DB already holds ' + JSON.stringify(f); });
  return db;
}
// after the launch's job: the run goes into the DB (the context's kept plan still holds it), the records are built from the metadata the job copied anyway
function collect_append(nat, ctx, db, res, files) {
  const r = nat.featdbAppendBatch(ctx, db.native);
  const level = db.level, step = settings.window_step / 1e3;
  const pos = new Uint32Array(res.meta.length / 8);          // a row's position in its callback: the rows before it with the same (clip, si)
  for (let q = 1; q < pos.length; q++) if (res.meta[q * 8] === res.meta[q * 8 - 8] && res.meta[q * 8 + 1] === res.meta[q * 8 - 7]) pos[q] = pos[q - 1] + 1;
  r.kept.forEach((src) => {
    if (level === 11) {
      const m = res.uttMeta.subarray(src * 4, src * 4 + 4);
      db.records.push({ file: files[m[0]], part: 0, time: [m[2] * step, (m[3] + 1) * step], truth: null, guess: null });
      return;
    }
    const m = res.meta.subarray(src * 8, src * 8 + 8);
    if (level === 5) db.records.push({ file: files[m[0]], part: m[1], time: [m[2] * step, (m[3] + 1) * step], truth: null, guess: null });
    else db.records.push({ file: files[m[0]], part: m[1] + pos[src] / 100, time: [(m[2] * step).toFixed(3), ((m[3] + 1) * step).toFixed(3)], truth: null, guess: null });
  });
  files.forEach((f) => db.files.add(f));
}
// what trainModel / trainRegression need of a device DB in place of prepared host rows: the selection as a row list and its ranges, taken on the device
function device_db_data(db, sel, n_labels) {
  live_device_db(db, 'trainModel');
  if (n_labels !== db.records.length) throw 'trainModel: ' + n_labels + ' labels for a device DB of ' + db.records.length + ' rows';
  const rows32 = Uint32Array.from(sel.rows);
  const rg = addon().featdbRanges(db.native, rows32);
  return Object.assign({}, sel, { db, rows32, inMin: rg.min, inMax: rg.max, width: db.width });
}

function LaunchAudioNodes(context_source, source_obj = null, callback = null, file_labels = [], offline = false,
  test_play = true, play_offset = null, play_duration = null) {
  return new Promise((resolve, reject) => {
    if (playing) { reject('Error: Already playing'); return; }
    let clip;
    try {
      if (context_source !== 1 || !source_obj) throw 'Invalid audio source';                  // ref @B5698
      clip = to_pcm(source_obj);
      if (play_offset || play_duration) {                                                     // bufferSource.start(0, offset, duration)
        const a = Math.max(0, Math.floor((play_offset || 0) * clip.sampleRate)), len = clip_length(clip);
        const b = play_duration ? Math.min(len, a + Math.floor(play_duration * clip.sampleRate)) : len;
        clip = clip_slice(clip, a, b);
      }
    } catch (e) { reject(typeof e === 'string' ? e : String(e.message || e)); return; }
    const ex = expand_channels([clip], [file_labels]);          // ('each': the channels' callbacks one after the other, file_labels.concat('ch' + c))
    run(ex.list, callback, (c) => ex.labels[c], test_play).then(() => resolve(true), (e) => reject(typeof e === 'string' ? e : String(e.message || e)));
  });
}

// extension: many independent clips in one GPU batch; callbacks are delivered clip by clip, in
// segment order, as callback(si, labels[clip], seg_time, features, clip_index)
function LaunchBatch(clips, callback = null, labels = [], test_play = false) {
  return new Promise((resolve, reject) => {
    let list;
    try { list = clips.map(to_pcm); } catch (e) { reject(typeof e === 'string' ? e : String(e.message || e)); return; }
    // configure({channel: 'each'}): the callbacks arrive in (clip, channel) order, clip_index counts the analyses
    ({ list, labels } = expand_channels(list, labels));
    let current = 0;
    const cb = callback ? (si, label, t, f) => callback(si, label, t, f, current) : null;
    const labels_of = (c) => { current = c; return labels[c] || []; };
    run(list, cb, labels_of, test_play).then((rs) => resolve(Object.assign({ rows: rs.reduce((t, r) => t + r.meta.length / 8, 0), segments: rs.reduce((t, r) => t + r.segments.length / 4, 0),
      stageMs: Array.from(rs[0].stageMs), shards: rs.length, stopped: stop_requested }, rs.meters ? { meters: rs.meters } : {}, rs.head_values ? { values: rs.head_values } : {},
      rs.min_entropy_db ? { min_entropy_db: rs.min_entropy_db, shown_min_entropy_db: rs.shown_min_entropy_db } : {})),
      (e) => reject(typeof e === 'string' ? e : String(e.message || e)));
  });
}

// extension: a SEQUENCE of batches, software-pipelined through two contexts on one device (each with its own planned batch and HIP stream, napi/wsa_napi.c):
// while batch k's kernels run, batch k + 1 uploads, and batch k - 1's callbacks are delivered on the JS thread.  The reference's app walks its files one launch
// at a time, the next one when the promise resolves (src/index.js:277-296) — a LaunchBatch per group of files, awaited one after the other, pays upload +
// kernels + callbacks in a row; this keeps the PCIe link busy instead (bench_host.js: i16p_sustained).  Callbacks arrive batch by batch, clip by clip, in segment
// order, as callback(si, labels[batch][clip], seg_time, features, clip_index, batch_index) — for every batch exactly what LaunchBatch delivers for it.
let pipe_cache = { key: null, ctxs: [] };
function pipe_contexts(nat) {
  const key = JSON.stringify([native_config(), settings.device]);
  if (pipe_cache.key !== key) {
    drop_pipe_contexts(nat);
    const ctxs = [];
    try { for (let i = 0; i < 2; i++) ctxs.push(nat.create(native_config(), settings.device)); }
    catch (e) { for (const c of ctxs) { try { nat.destroy(c); } catch (e2) { /* first error wins */ } } throw e; }
    pipe_cache = { key, ctxs };
  }
  return pipe_cache.ctxs;
}
function drop_pipe_contexts(nat) {
  for (const c of pipe_cache.ctxs) knn_natives.delete(c);
  for (const c of pipe_cache.ctxs) { try { nat.destroy(c); } catch (e) { /* a failed launch's straggler still uses it: left to process exit */ } }
  pipe_cache = { key: null, ctxs: [] };
}
async function run_batches(batches, callback, labels, test_play) {
  const nat = addon();
  if (playing) throw 'Error: Already playing';                                               // ref @B4554
  playing = true; stop_requested = false; labels_per_segment = [];
  try {
    // a collecting DB lives on one context: its batches run there one after the other
    const cdb = collect_db ? live_device_db(collect_db, 'setCollectDB') : null;
    const ctxs = cdb ? [cdb.ctx, cdb.ctx] : pipe_contexts(nat);
    const pred = prediction && settings.output_level === 13 ? prediction : null;
    const models = ctxs.map((c) => (pred ? model_on(nat, c) : undefined));
    const vp = value_prediction && settings.output_level === 13 ? value_prediction : null;
    const meters = pred ? [] : null;
    const mdbs = pred && pred.models ? [] : null;          // per batch and clip: the clip's min_entropy_db (null: none)
    const vals = vp ? [] : null;                           // per batch and clip: the value heads' {sum, weight, value}
    if (settings.channel !== 'first') throw "LaunchBatches analyses channel 0: configure({channel: 'first'}), or LaunchBatch for '" + settings.channel + "'";
    const lists = batches.map((b) => b.map(to_pcm));
    const bands = settings.spec_type === 1 ? settings.N_mel_bins : settings.N_fft_bins;
    const start = (k) => {
      const clips = lists[k];
      const rates = new Set(clips.map((c) => c.sampleRate));
      if (rates.size !== 1 && !(settings.resample_to > 0)) throw 'All clips of one launch must share a sample rate';
      const fs = rates_of(clips), fs_an = settings.resample_to > 0 ? settings.resample_to : clips[0].sampleRate;
      const g = nat.geometry(ctxs[k % 2], fs_an);
      if (g.bands !== bands) throw 'Bins count mismatch: ' + g.bands + ', ' + bands;          // ref @B8568 check
      const extra = pred && !pred.knn ? [models[k % 2]] : [];
      if (cdb) collect_check(ctxs[0], clips.map((_, c) => ((labels[k] || [])[c] || [])[0]));
      return submit_clips(nat, ctxs[k % 2], clips, fs, fs_an, false, extra);
    };
    let rows = 0, segments = 0, done = 0;
    let next = lists.length > 0 ? start(0) : null;
    for (let k = 0; k < lists.length; k++) {
      const mine = next;
      // batch k + 1 goes to the other context now (its previous job, batch k - 1, was awaited one turn ago); a failure to start it must not leave batch k unawaited
      let start_err = null;
      next = null;
      if (!cdb && k + 1 < lists.length && !stop_requested) { try { next = start(k + 1); } catch (e) { start_err = e; } }
      let res;
      try { res = await mine; }
      catch (e) { if (next) { try { await next; } catch (e2) { /* the first failure is reported */ } } if (!cdb) drop_pipe_contexts(nat); throw e; }
      if (start_err) { drop_pipe_contexts(nat); throw start_err; }     // (only without a collecting DB: with one, nothing was started above)
      // the run goes into the DB before the context's next batch reuses its tables (that batch starts below, behind the folds that read the same tables)
      if (cdb) collect_append(nat, ctxs[0], cdb, res, lists[k].map((_, c) => ((labels[k] || [])[c] || [])[0]));
      if (pred && pred.knn) {               // (context k % 2 is idle until batch k + 2 starts)
        try { knn_fold_into(nat, ctxs[k % 2], res, pred); } catch (e) { if (next) { try { await next; } catch (e2) { /* the first failure is reported */ } } if (!cdb) drop_pipe_contexts(nat); throw e; }
      }
      if (vp) {                             // (likewise)
        try { values_fold_into(nat, ctxs[k % 2], res, vp); } catch (e) { if (next) { try { await next; } catch (e2) { /* the first failure is reported */ } } if (!cdb) drop_pipe_contexts(nat); throw e; }
      }
      if (cdb && k + 1 < lists.length && !stop_requested) next = start(k + 1);       // (a collecting DB's context is free again: nothing is in flight if this throws)
      rows += res.meta.length / 8; segments += res.segments.length / 4; done++;
      if (!test_play && (callback || pred || vp) && !stop_requested) {                              // ref @B24762: silent when test_play
        const lb = labels[k] || [];
        for (let c = 0; c < lists[k].length && !stop_requested; c++) {
          const cb = callback ? (si, label, t, f) => callback(si, label, t, f, c, k) : null;
          const pk = pred ? { model: pred.model, models: pred.models, state: pred.state, on_prediction: (si, lc, ci, per) => pred.on_prediction(si, lc, ci, per, k) } : null;
          const vk = vp ? { on_values: (si, v, ci, detail) => vp.on_values(si, v, ci, detail, k) } : null;
          dispatch(res, c, cb, lb[c] || [], pk, c, vk);
        }
      }
      if (vals) vals.push(Array.from({ length: lists[k].length }, (_, c) => clip_values_of(res.reg, c)));
      if (meters) meters.push(Array.from({ length: lists[k].length }, (_, c) => (pred.models ? ensemble_meters_of(res, c, pred, res.ensAccs) : meters_of(res, c, pred.model.labels))));
      if (mdbs) mdbs.push(Array.from(res.ens.minDb.subarray(0, lists[k].length), (v) => (v >= 0 ? v : null)));
      if (stop_requested && next) { try { await next; } catch (e) { /* stopping */ } next = null; done++; break; }
    }
    return Object.assign({ rows, segments, batches: done, stopped: stop_requested }, meters ? { meters } : {},
      vals ? { values: vals } : {}, mdbs ? { min_entropy_db: mdbs, shown_min_entropy_db: pred.state.min_db } : {});
  } finally {
    playing = false;
  }
}
function LaunchBatches(batches, callback = null, labels = [], test_play = false) {
  return new Promise((resolve, reject) => {
    if (!Array.isArray(batches) || batches.some((b) => !Array.isArray(b) || b.length === 0)) { reject('LaunchBatches(batches: clip[][], callback, labels[][][])'); return; }
    run_batches(batches, callback, labels, test_play).then(resolve, (e) => reject(typeof e === 'string' ? e : String(e.message || e)));
  });
}

// extension: n concurrent real-time streams in lock step (the reference's online path — worklet frame ->
// spectrum_push with carried state -> callback as a segment closes, ref @B8752 / @B28869 — for many
// sources at once).  Returns {input, samplesPerStep, push(ctl), close()}: write each stream's next
// samplesPerStep samples into input (a Float32Array over the pinned [n][samplesPerStep] buffer), call
// push(); callbacks fire as callback(si, labels[stream], seg_time, features, stream) for every segment that
// closed in that step.  ctl = Uint8Array of STREAM_ACTIVE | STREAM_START | STREAM_STOP per stream, or
// omitted (all streams start on the first push and stay active).
// With a prediction model set (setPredictionModel) when a level-13 stream object opens, its steps classify their syllables on the GPU:
// on_prediction(si, [label, confidence], stream, per_syllable) follows each callback (as for LaunchBatch, the stream in place of the clip),
// and push() / close() return `meters`, one {label: Label_conf_all} per stream (reset by the stream's START).  The object keeps the model it
// opened with until close().
// sample_rate may be an array with one rate per stream.  With configure({resample_to: R}), R > 0, every stream is converted from its own rate to R
// inside the step (spec RS-1, as LaunchBatch converts clips; geometry, bins_Hz and the band check come from R) and streams already at R pass
// unfiltered; without it the streams must share a rate.  The handle of a converting set also has `capacity` (Uint32Array: the samples one push
// accepts per stream), `inputStride` (floats per stream in `input`: stream i's samples of a push start at input[i * inputStride]), paced() (what a
// push without counts takes from every stream next: what keeps it on real time) and push(ctl, counts) with counts = Uint32Array of samples per
// stream.  samplesPerStep keeps its meaning: frames_per_step * hop samples at the analysis rate.  The reference's live path runs at the hardware's
// rate and converts nothing; this is ours, like resample_to.
const STREAM_ACTIVE = 1, STREAM_START = 2, STREAM_STOP = 4;
// The seventh argument (optional) = {format: 'f32' | 'i16' | 'mulaw' | 'alaw', channels}: the sources hand over packed PCM (spec PK-1), unpacked
// on the GPU inside the step.  handle.input is then an Int16Array ('i16') or Uint8Array (G.711) over the packed pinned buffer, handle.inputStride
// counts elements of that array, stream i's frames of a push are interleaved over channels (a number, or one per stream; 1 .. 64) from
// input[i * inputStride] on and channel 0 is analysed.  push(ctl, counts) is unchanged: counts are frames of one channel.
// With select ('mix' or a channel number, one value or one per stream) and / or source (one stream index per stream) stream i analyses that channel, or the
// mono mix, of the row of stream source[i] (spec PK-3): a stereo call is written once, into its source's row, and feeds a stream per speaker.
const PCM_FORMATS = { f32: 0, i16: 1, mulaw: 2, alaw: 3 };
function pcm_format(format) {
  if (!Object.prototype.hasOwnProperty.call(PCM_FORMATS, format)) throw "unknown input format '" + format + "' ('f32', 'i16', 'mulaw', 'alaw')";
  return PCM_FORMATS[format];
}
// channel `select` (0; 'mix': the mono mix, spec PK-3) of the interleaved frames in typedArray as the floats the analysis is given (Int16Array for 'i16',
// Uint8Array for 'mulaw' / 'alaw')
function channel_select(select) {
  if (select === 'mix') return CHANNEL_MIX;
  if (!(Number.isInteger(select) && select >= 0 && select <= CHANNEL_MIX)) throw "select: a channel number or 'mix'";
  return select;
}
function decodePcm(format, typedArray, channels = 1, select = 0) {
  try { return addon().decodePcm(pcm_format(format), typedArray, channels, channel_select(select)); } catch (e) { throw (typeof e === 'string' ? e : String(e.message || e)); }
}
// The eighth argument (optional) = {collect: db, names: [one per stream]}: every push appends the step's vectors to the device DB `db` (createDeviceDB)
// on the GPU, inside the step (spec FD-2), by the app's storing rules; names[i] is the "file" of stream i's launch (default labels[i][0], as the
// collector of js/featuredb.js takes it; handle.rename(i, name) names the launch its next START begins).  db.records grows per push as it does per
// batch; at level 11 a launch owns one record, rewritten by every later result.  Without the argument the DB given to setCollectDB collects the sets
// opened from then on.  The set then runs on the DB's context (a DB lives in one context): refused like setCollectDB with several devices or another
// level.  db.count() and db.toFeatureDB() are for after handle.close(): the addon refuses them while the context has an open stream set.
function stream_collect_db(opts, n_streams, labels) {
  const db = opts && opts.collect ? opts.collect : (opts ? null : collect_db);
  if (!db) return null;
  live_device_db(db, 'StreamOpen');
  if (several_devices()) throw several_devices_message();
  if (db.level !== settings.output_level) throw 'StreamOpen: the DB holds the vectors of output_level ' + db.level + ', the streams run at ' + settings.output_level;
  const names = opts && opts.names ? Array.from(opts.names, String) : Array.from({ length: n_streams }, (_, i) => (labels[i] || [])[0]);
  if (names.length !== n_streams || names.some((f) => f === undefined)) throw 'StreamOpen: names holds one name per stream (' + n_streams + ' streams)';
  names.forEach((f, i) => { if (db.files.has(f) || names.indexOf(f) < i) throw 'StreamOpen: the DB already holds ' + JSON.stringify(f); });
  return { db, names };
}
function StreamOpen(n_streams, sample_rate, callback = null, labels = [], frames_per_step = 1, max_span_frames = 1024, input_format = null, collect = undefined) {
  const nat = addon();
  const level = settings.output_level, step = settings.window_step / 1e3;
  const cdb = stream_collect_db(collect, n_streams, labels);
  if (![3, 4, 5, 10, 11, 12, 13].includes(level)) throw 'output_level ' + level + ' is not available for streams through this build (3, 4, 5, 10, 11, 12 and 13 are)';
  const per_stream = Array.isArray(sample_rate) || ArrayBuffer.isView(sample_rate);
  if (per_stream && sample_rate.length !== n_streams) throw 'sample_rate as an array holds one rate per stream (' + sample_rate.length + ' rates, ' + n_streams + ' streams)';
  const rates = per_stream ? Array.from(sample_rate) : [sample_rate];
  const convert = settings.resample_to > 0;
  if (new Set(rates).size !== 1 && !convert) throw 'All streams of one set must share a sample rate (configure resample_to to convert each from its own)';
  const fs_an = convert ? settings.resample_to : rates[0];      // the rate the analysis runs at (K0s converts inside the step)
  const pred = prediction && level === 13 ? prediction : null;
  const vp = value_prediction && level === 13 ? value_prediction : null;
  const ctx = cdb ? cdb.db.ctx : nat.create(native_config(), settings.device);      // a collecting set runs on its DB's context, which stays when the set closes
  let st;
  try {
    const g = nat.geometry(ctx, fs_an);
    const bands = settings.spec_type === 1 ? settings.N_mel_bins : settings.N_fft_bins;
    if (g.bands !== bands) throw 'Bins count mismatch: ' + g.bands + ', ' + bands;              // ref @B8568 check
    st = convert ? nat.streamOpenMixed(ctx, n_streams, Float64Array.from(per_stream ? rates : new Array(n_streams).fill(rates[0])), fs_an, frames_per_step, max_span_frames)
      : nat.streamOpen(ctx, n_streams, rates[0], frames_per_step, max_span_frames);
    if (input_format) {
      const chans = input_format.channels;
      const ch = chans === undefined || chans === null ? null : Uint32Array.from(Array.isArray(chans) || ArrayBuffer.isView(chans) ? chans : new Array(n_streams).fill(chans));
      if (ch && ch.length !== n_streams) throw 'channels as an array holds one count per stream (' + ch.length + ' counts, ' + n_streams + ' streams)';
      // select / source (spec PK-3): what each stream takes ('mix' or a channel, one value or one per stream) of which stream's packed row
      const per = (v, what) => {
        if (v === undefined || v === null) return null;
        const a = Array.isArray(v) || ArrayBuffer.isView(v) ? Array.from(v) : new Array(n_streams).fill(v);
        if (a.length !== n_streams) throw what + ' as an array holds one entry per stream (' + a.length + ' entries, ' + n_streams + ' streams)';
        return a;
      };
      const sel = per(input_format.select, 'select'), src = per(input_format.source, 'source');
      if (sel || src) nat.streamSetInput(st, pcm_format(input_format.format === undefined ? 'f32' : input_format.format), ch, sel ? Uint32Array.from(sel, channel_select) : null, src ? Uint32Array.from(src) : null);
      else nat.streamSetInput(st, pcm_format(input_format.format === undefined ? 'f32' : input_format.format), ch);
    }
    if (pred && pred.knn) nat.streamSetKnn(st, knn_store_on(nat, ctx, pred.knn), pred.k);
    else if (pred && pred.models) nat.streamSetEnsemble(st, model_on(nat, ctx));
    else if (pred) nat.streamSetModel(st, model_on(nat, ctx));       // the native model on the stream's own context (ref src/index.js:56)
    if (vp) nat.streamSetRegress(st, ...value_heads_on(nat, ctx, vp));
    if (cdb) { nat.streamSetFeatdb(st, cdb.db.native); cdb.names.forEach((f) => cdb.db.files.add(f)); }
  } catch (e) {
    if (st) nat.streamClose(st);
    if (!cdb) {
      if (pred) forget_natives(pred, ctx);
      if (vp) for (const h of vp.models) h.natives.delete(ctx);
      nat.destroy(ctx);
    }
    throw (typeof e === 'string' ? e : String(e.message || e));
  }
  const packed = !!input_format && input_format.format !== undefined && input_format.format !== 'f32';
  const input = nat.streamInput(st);
  const info = convert || packed ? nat.streamInfo(st) : null;
  if (packed) info.inputStride = info.inputStrideBytes / input.BYTES_PER_ELEMENT;
  const names = pred && pred.knn ? pred.knn.names.slice() : null;       // a KNN store: the labels of the rows the set opened with
  // the step's KNN tables under the names predict_after and meters_of read a model's by
  const knn_view = (res) => ({ cb: res.knnCb, cbLabel: res.knnCbLabel, cbConf: res.knnCbConf, prob: res.knnConf, nClasses: res.knnNClasses });
  const spred = pred && pred.knn ? { model: { labels: names }, on_prediction: pred.on_prediction } : pred && pred.models ? { models: pred.models, state: pred.state, on_prediction: pred.on_prediction, accs: new Map() } : pred;   // accs: per stream, since its START
  const reg_accs = new Map();                         // value heads: RG-1's running sums per stream, since its START
  const reg_view = (res) => ({ cb: res.regCb, cbValue: res.regCbValue, cbWeight: res.regCbWeight, value: res.regValue, nHeads: res.regNHeads });
  let values = null;                                    // ... and of the value heads
  let open = true, started = false, meters = null;      // meters: the per-stream Label_conf_all of the last step (a prediction model only)
  const stopped = new Uint8Array(n_streams);          // streams that have had their segment_truncate since their last START
  const seg_seen = new Uint32Array(n_streams);        // level 3: segments a stream has closed since its last START (the callback index, ref @B28273)
  const feat = (res, r) => Array.from(res.feat.subarray(r * 53, r * 53 + 53));
  const deliver = (res) => {
    const rows = res.meta.length / 8;
    if (level === 3) {
      // the ranked raw tracks of every segment that closed (ref @B28273, @B30132: no fourth argument); the stream is the fifth argument as at every level
      for (let k = 0; k < res.segments.length / 4; k++) {
        const s = res.segments[4 * k], tr = callback ? tracks_of_segment(res, k) : [];
        if (tr.length > 0) callback(seg_seen[s], labels[s] || [], tr, undefined, s);
        seg_seen[s]++;
      }
    } else if (callback && level === 11) {
      // utterance features: after every result the 264 histogram bins over everything the source has produced so far, callback index 0 (ref @B28869)
      for (let k = 0; k < res.uttMeta.length / 4; k++) {
        const m = res.uttMeta.subarray(k * 4, k * 4 + 4);
        callback(0, labels[m[0]] || [], [m[2] * step, (m[3] + 1) * step], Array.from(res.uttFeat.subarray(k * 264, k * 264 + 264)), m[0]);   // ref Y() @B31330
      }
    } else if (callback || ((pred || vp) && level === 13)) {
      let r = 0;
      while (r < rows) {
        const s = res.meta[r * 8], si = res.meta[r * 8 + 1];
        // levels 4 / 10: the straightened frames of the row's segment / syllable, Float32Array(9) per frame (ref @B35074)
        const frames = (k) => { const o = []; for (let q = res.formantOff[k]; q < res.formantOff[k + 1]; q++) o.push(res.formants.slice(9 * q, 9 * q + 9)); return o; };
        if (level === 5 || level === 4) {
          callback(si, labels[s] || [], [res.meta[r * 8 + 2] * step, (res.meta[r * 8 + 3] + 1) * step], level === 5 ? feat(res, r) : frames(r), s);   // ref @B29622, @B31504, @B28124
          r++;
        } else if (level === 10) {
          const times = [], syl = [];
          while (r < rows && res.meta[r * 8] === s && res.meta[r * 8 + 1] === si) {
            times.push([(res.meta[r * 8 + 2] * step).toFixed(3), ((res.meta[r * 8 + 3] + 1) * step).toFixed(3)]);
            syl.push(frames(r)); r++;
          }
          callback(si, labels[s] || [], times, syl, s);                                                                        // ref @B27713
        } else {
          // level 13: 53 features per syllable; level 12: the 23 polynomial numbers, the list ending at a syllable on which numeric threw
          const times = [], feats = [];
          let cut = false;
          while (r < rows && res.meta[r * 8] === s && res.meta[r * 8 + 1] === si) {
            times.push([(res.meta[r * 8 + 2] * step).toFixed(3), ((res.meta[r * 8 + 3] + 1) * step).toFixed(3)]);             // ref @B31114
            if (level === 12 && res.feat[r * 53 + 23] !== 0) cut = true;
            if (!cut) feats.push(level === 12 ? Array.from(res.feat.subarray(r * 53, r * 53 + 23)) : feat(res, r));
            r++;
          }
          if (feats.length > 0) {
            if (callback) callback(si, labels[s] || [], times, feats, s);                                                      // ref @B29138 (`p[e].length>0`)
            if (pred && pred.knn) { if (res.knnCb) { res.knnView = res.knnView || knn_view(res); predict_after(res.knnView, r - times.length, si, s, spred); } }
            else if (pred && has_cb(res) && level === 13) predict_after(res, r - times.length, si, s, spred);                         // ref prediction.js:70
            if (vp && res.regCb) { res.regView = res.regView || reg_view(res); values_after(res.regView, res.meta, r - times.length, si, s, vp, reg_accs); }
          }
        }
      }
    }
    if (cdb) collect_step(res);
    const out = { rows, segments: res.segments.length / 4, cuts: res.cuts, cut: (res.flags & 8) !== 0, dbFull: (res.flags & 16) !== 0 };   // dbFull: the step's vectors did not fit the collecting DB (WSA_FLAG_DB_FULL); cut: some stream's span reached max_span_frames in this step (WSA_FLAG_STREAM_CUT)
    if (pred && pred.knn) {
      if (res.knnStreamConf) meters = out.meters = Array.from({ length: n_streams }, (_, s) => meters_of({ nClasses: res.knnNClasses, clipConf: res.knnStreamConf }, s, names));
    } else if (pred && pred.models && res.ens && res.ens.cb) {
      meters = out.meters = Array.from({ length: n_streams }, (_, s) => ensemble_meters_of(res, s, pred, spred.accs));
      out.min_entropy_db = Array.from(res.ens.minDb, (v) => (v >= 0 ? v : null));
      out.shown_min_entropy_db = pred.state.min_db;
    } else if (pred && res.streamConf) meters = out.meters = Array.from({ length: n_streams }, (_, s) => meters_of({ nClasses: res.nClasses, clipConf: res.streamConf }, s, pred.model.labels));
    if (vp && res.regRunValue) {        // per stream: the device's running sums and value of every head
      const H = res.regNHeads, at = (t, s) => Array.from({ length: H }, (_, h) => t[h * n_streams + s]);
      values = out.values = Array.from({ length: n_streams }, (_, s) => ({ sum: at(res.regSum, s), weight: at(res.regWeight, s), value: at(res.regRunValue, s) }));
    }
    return out;
  };
  // FD-2's host half: the step's kept / replaced lists become the DB's records, shaped as collect_append shapes a batch's
  const next_names = new Map();
  const collect_step = (res) => {
    const d = nat.streamDbRows(st), db = cdb.db;
    const pos = new Uint32Array(res.meta.length / 8);
    for (let q = 1; q < pos.length; q++) if (res.meta[q * 8] === res.meta[q * 8 - 8] && res.meta[q * 8 + 1] === res.meta[q * 8 - 7]) pos[q] = pos[q - 1] + 1;
    const record = (src) => {
      if (level === 11) { const m = res.uttMeta.subarray(src * 4, src * 4 + 4); return { file: cdb.names[m[0]], part: 0, time: [m[2] * step, (m[3] + 1) * step], truth: null, guess: null }; }
      const m = res.meta.subarray(src * 8, src * 8 + 8);
      if (level === 5) return { file: cdb.names[m[0]], part: m[1], time: [m[2] * step, (m[3] + 1) * step], truth: null, guess: null };
      return { file: cdb.names[m[0]], part: m[1] + pos[src] / 100, time: [(m[2] * step).toFixed(3), ((m[3] + 1) * step).toFixed(3)], truth: null, guess: null };
    };
    if (d.first !== db.records.length && d.added) throw 'StreamOpen: the collecting DB holds ' + db.records.length + ' records, the step stored from row ' + d.first;
    d.kept.forEach((src) => db.records.push(record(src)));
    for (let q = 0; q < d.replaced; q++) Object.assign(db.records[d.replacedRows[2 * q + 1]], { time: record(d.replacedRows[2 * q]).time });
  };
  const handle = {
    input, samplesPerStep: info ? info.samplesPerStep : input.length / n_streams, stopPending: false,
    rename(i, name) {
      if (!cdb) throw 'rename: this stream set collects into no device DB';
      name = String(name);
      if (cdb.db.files.has(name)) throw 'StreamOpen: the DB already holds ' + JSON.stringify(name);
      if (next_names.has(i)) cdb.db.files.delete(next_names.get(i));
      next_names.set(i, name); cdb.db.files.add(name);
    },
    push(ctl = null, counts = null) {
      if (!open) throw 'stream closed';
      // StopAudioNodes (ref @B5699 -> disconnect_nodes @B21559): the frame in flight is still pushed, then every source is truncated
      // (segment_truncate, ref @B8851 / @B30757) — the open segments are flushed and reported, the object closes
      const c = new Uint8Array(n_streams);
      for (let i = 0; i < n_streams; i++) {
        c[i] = ctl ? ctl[i] : (STREAM_ACTIVE | (started ? 0 : STREAM_START));
        if (handle.stopPending && !stopped[i]) c[i] |= STREAM_STOP;
        if ((c[i] & STREAM_START) && next_names.has(i)) { cdb.names[i] = next_names.get(i); next_names.delete(i); }
        if (c[i] & STREAM_START) { stopped[i] = 0; seg_seen[i] = 0; if (spred && spred.accs) spred.accs.delete(i); reg_accs.delete(i); }
        if (c[i] & STREAM_STOP) stopped[i] = 1;
      }
      started = true;
      const out = deliver(counts ? nat.streamStep(st, c, counts instanceof Uint32Array ? counts : Uint32Array.from(counts)) : nat.streamStep(st, c));
      if (handle.stopPending) handle.close(false);
      return out;
    },
    // flush = true: sources that have not been stopped yet get their segment_truncate first (a step without new frames), so that the
    // segment a source is in the middle of is reported like the reference reports it when its nodes are disconnected
    close(flush = true) {
      if (!open) return { rows: 0, segments: 0 };
      let out = Object.assign({ rows: 0, segments: 0 }, meters ? { meters } : {}, values ? { values } : {});
      if (flush && started && stopped.some((v) => !v)) {
        const c = new Uint8Array(n_streams);
        for (let i = 0; i < n_streams; i++) if (!stopped[i]) { c[i] = STREAM_STOP; stopped[i] = 1; }
        out = deliver(nat.streamStep(st, c));
      }
      open = false; open_streams.delete(handle);
      nat.streamClose(st);                             // detaches `input`: the pinned buffer is gone; releases the model; the collecting DB is attached to nothing
      if (!cdb) {
        if (pred) forget_natives(pred, ctx);            // the native models go with the stream's context
        if (vp) for (const h of vp.models) h.natives.delete(ctx);
        nat.destroy(ctx);
      }
      return out;
    },
  };
  if (info) Object.assign(handle, { capacity: info.capacity, inputStride: info.inputStride, paced: () => nat.streamPaced(st) });
  open_streams.add(handle);
  return handle;
}

// ref @B5699 -> disconnect_nodes @B21559 (`0 != audioPlaying && (audioPlaying = -1)`): only a running analysis is affected.  A batch
// launch stops dispatching and resolves; open stream objects flush their sources at their next push() and close.
function StopAudioNodes(reason = 'no reason') {
  if (playing) stop_requested = true;
  for (const h of open_streams) h.stopPending = true;
}

function set_predicted_label_for_segment(si, idx, label) {                                    // ref @B31711
  if (!labels_per_segment[si]) labels_per_segment[si] = [];
  while (labels_per_segment[si].length < idx) labels_per_segment[si].push(-1);
  labels_per_segment[si][idx] = label;
}

module.exports = { configure, LaunchAudioNodes, StopAudioNodes, set_predicted_label_for_segment, LaunchBatch, LaunchBatches,
  StreamOpen, decodePcm, STREAM_ACTIVE, STREAM_START, STREAM_STOP, shutdown, allocPinned, freePinned,
  _settings: settings, _decode_wav: decode_wav, _clip_floats: clip_floats, _clip_length: clip_length, _values_after: values_after, loadModel, setPredictionModel, setPredictionModels, setPredictionKnn, setPredictionValues, trainModel, trainModels, saveModel, trainRegression, predictValues, predictDB, statsTable, evaluateDB, crossValidate,
  KNNClassifier, trainKnn, predictKnn, createDeviceDB, setCollectDB };
