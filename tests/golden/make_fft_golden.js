#!/usr/bin/env node
// Records golden events and outputs of the `fft` analyzer node (wasm/FFT.h) from the reference's own prebuilt wasm engine
// (js/packages/offline-renderer/elementary-wasm.cjs: Runtime<double>, FFTNode<double> — the window is made and applied in
// double, the product rounded to float32, then audiofft's float transform).
//
// Authoring container only:  node tests/golden/make_fft_golden.js
// (same textual patch of a TEMP copy of the emscripten glue as make_convolve_golden.js: Node 12 cannot parse its ES2020 syntax)
// Output: tests/golden/fft_wasm.f32  little-endian float32: per scenario the first `out_stored` output frames of every channel,
//                                    then real[size/2+1] | imag[size/2+1] of every STORED event
//         tests/golden/fft_wasm.json scenarios (what was driven, every event's block / source / size / first input frame, offsets
//                                    of the stored ones), E_ref per size, the rejected-property results.
// E_ref[size] = max |recorded bin - float64 DFT bin| over every bin of every event of that size (stored or not), the DFT taken
// of the float32 windowed frame the node transformed. The script finds that frame itself by replaying MultiChannelRingBuffer's
// positions over the input it fed; a wrong replay shows as an E_ref of the size of the spectrum and stops the script.
const fs = require('fs'), os = require('os'), path = require('path');
const HERE = __dirname;
const REF = '/root/reference/js/packages/offline-renderer/elementary-wasm.cjs';

function patchedGlue() {
  let src = fs.readFileSync(REF, 'utf8');
  src = src.replace(/globalThis\?\.crypto\?\.getRandomValues/g, '(globalThis.crypto&&globalThis.crypto.getRandomValues)');
  src = src.replace(/([A-Za-z_$][\w$]*(?:\.[A-Za-z_$][\w$]*)+)\?\.\(([^()]*)\)/g, (m, f, a) => `(${f}&&${f}(${a}))`);
  src = src.replace(/([A-Za-z_$][\w$]*)\?\?=([\w$]+)/g, (m, v, d) => `${v}=(${v}==null?${d}:${v})`);
  src = src.replace(/([A-Za-z_$][\w$]*)&&=([A-Za-z_$][\w$]*\([^()]*\))/g, (m, v, e) => `${v}=${v}&&(${e})`);
  src = src.replace(/\(X=C\.U\)\.ka\?\?\(X\.ka=\[\]\)/g, '((X=C.U).ka!=null?X.ka:(X.ka=[]))');
  const out = path.join(fs.mkdtempSync(path.join(os.tmpdir(), 'elemwasm-')), 'elementary-wasm.patched.cjs');
  fs.writeFileSync(out, src);
  return out;
}

function Lcg(seed) { let s = seed >>> 0; return () => { s = (Math.imul(1664525, s) + 1013904223) >>> 0; return s / 2147483648 - 1; }; }

// FFT.h:51-65 with FloatType = double
function windowOf(size) {
  const w = new Float64Array(size);
  for (let i = 0; i < size; ++i) {
    const t = i / (size - 1);
    w[i] = 0.35875 - 0.48829 * Math.cos(2.0 * Math.PI * t) + 0.14128 * Math.cos(4.0 * Math.PI * t) - 0.01168 * Math.cos(6.0 * Math.PI * t);
  }
  return w;
}

// float64 DFT of a real frame: bins 0 .. size/2 (forward sign, unnormalised)
function dft(frame) {
  const S = frame.length, c = new Float64Array(S), s = new Float64Array(S);
  for (let j = 0; j < S; ++j) { c[j] = Math.cos(2.0 * Math.PI * j / S); s[j] = Math.sin(2.0 * Math.PI * j / S); }
  const re = new Float64Array(S / 2 + 1), im = new Float64Array(S / 2 + 1);
  for (let k = 0; k <= S / 2; ++k) {
    let a = 0.0, b = 0.0;
    for (let n = 0; n < S; ++n) { const j = (n * k) & (S - 1); a += frame[n] * c[j]; b -= frame[n] * s[j]; }
    re[k] = a; im[k] = b;
  }
  return { re, im };
}

// MultiChannelRingBuffer.h:34-91 over ABSOLUTE frame numbers of the input (a frame below 0: the ring's initial zeros)
class RingModel {
  constructor() { this.W = 0; this.R = 0; }
  pos(a) { return ((a % 8192) + 8192) % 8192; }
  write(n) {
    const w = this.pos(this.W), r = this.pos(this.R);
    const free = r > w ? r - w : 8192 - (w - r);
    if (n >= free) this.R = this.W + n + 1 - 8192;
    this.W += n;
  }
  read(size) {
    const w = this.pos(this.W), r = this.pos(this.R);
    const full = w > r ? w - r : (8192 - (r - w)) & 8191;
    if (full < size) return -1;
    const at = this.R;
    this.R += size;
    return at;
  }
}

// graph 'single': root(1) <- fft(2) <- in(3);  graph 'pair': root(1, ch 0) <- fft(2) <- in(3), root(4, ch 1) <- meter(5) <- fft(6) <- in(3)
const SCENARIOS = [
  { name: 'a_default', graph: 'single', block: 512, blocks: 40, ffts: [{ id: 2, props: {} }], store: (e, n) => e < 8 || e === n - 1 },
  { name: 'b_size256', graph: 'single', block: 512, blocks: 40, ffts: [{ id: 2, props: { size: 256 } }], store: (e, n) => e < 10 || e >= n - 10 },
  { name: 'c_size4096', graph: 'single', block: 512, blocks: 64, ffts: [{ id: 2, props: { size: 4096 } }], store: (e, n) => e < 2 || e === n - 1 },
  { name: 'd_size8192', graph: 'single', block: 512, blocks: 40, ffts: [{ id: 2, props: { size: 8192 } }], store: () => true },
  { name: 'e_size2048_block128', graph: 'single', block: 128, blocks: 64, ffts: [{ id: 2, props: { size: 2048 } }], store: () => true },
  { name: 'f_size2048_block1024', graph: 'single', block: 1024, blocks: 16, ffts: [{ id: 2, props: { size: 2048 } }], store: (e, n) => e < 4 || e === n - 1 },
  { name: 'g_size1024_then512', graph: 'single', block: 512, blocks: 20, ffts: [{ id: 2, props: { size: 1024 } }],
    changes: [{ after_block: 9, id: 2, key: 'size', value: 512 }], store: () => true },
  { name: 'h_size512_every3rd', graph: 'single', block: 512, blocks: 36, relay_every: 3, ffts: [{ id: 2, props: { size: 512 } }], store: () => true },
  { name: 'i_two_and_a_meter', graph: 'pair', block: 512, blocks: 12,
    ffts: [{ id: 2, props: { name: 'a', size: 512 } }, { id: 6, props: { name: 'b', size: 2048 } }], meter: { id: 5, props: { name: 'm' } }, store: () => true },
];
const OUT_STORED = 1024;   // the root's 20 ms fade-in ends at frame 960: from there on the output IS the input, bit for bit (checked)
const INPUT_SEED = 11, INPUT_AMP = 0.5;

function batchOf(sc) {
  const b = [[0, 1, 'root'], [0, 2, 'fft'], [0, 3, 'in'], [3, 3, 'channel', 0], [3, 1, 'channel', 0]];
  if (sc.graph === 'pair') b.push([0, 4, 'root'], [0, 5, 'meter'], [0, 6, 'fft'], [3, 4, 'channel', 1]);
  for (const f of sc.ffts) for (const k of Object.keys(f.props)) b.push([3, f.id, k, f.props[k]]);
  if (sc.meter) for (const k of Object.keys(sc.meter.props)) b.push([3, sc.meter.id, k, sc.meter.props[k]]);
  b.push([2, 2, 3, 0], [2, 1, 2, 0]);
  if (sc.graph === 'pair') b.push([2, 6, 3, 0], [2, 5, 6, 0], [2, 4, 5, 0]);
  b.push([4, sc.graph === 'pair' ? [1, 4] : [1]], [5]);
  return b;
}

(async () => {
  const M = await require(patchedGlue())();
  const chunks = [], manifest = { sample_rate: 48000, input_seed: INPUT_SEED, input_amp: INPUT_AMP, out_stored: OUT_STORED, scenarios: {}, E_ref: {}, peak: {}, rejected: [] };
  let offset = 0;
  const push = (f32) => { chunks.push(Buffer.from(f32.buffer, f32.byteOffset, f32.byteLength)); const at = offset; offset += f32.length; return at; };
  for (const sc of SCENARIOS) {
    const nOut = sc.graph === 'pair' ? 2 : 1, total = sc.block * sc.blocks;
    const p = new M.ElementaryAudioProcessor(1, nOut);
    p.prepare(48000, sc.block);
    let r = p.postMessageBatch(batchOf(sc));
    if (!r.success) throw new Error(sc.name + ': ' + r.message);
    const next = Lcg(INPUT_SEED), x = new Float32Array(total);
    for (let j = 0; j < total; ++j) x[j] = Math.fround(next() * INPUT_AMP);
    const sizeOf = {}, ring = {}, nameOf = {};
    for (const f of sc.ffts) { sizeOf[f.id] = f.props.size === undefined ? 1024 : f.props.size; ring[f.id] = new RingModel(); nameOf[f.id] = f.props.name === undefined ? null : f.props.name; }
    const outs = []; for (let c = 0; c < nOut; ++c) outs.push(new Float32Array(total));
    const events = [];   // {type, block, source, size, frame, re, im} | {type: 'meter', block, source}
    const every = sc.relay_every || 1;
    for (let b = 0; b < sc.blocks; ++b) {
      const inp = p.getInputBufferData(0);
      for (let j = 0; j < sc.block; ++j) inp[j] = x[b * sc.block + j];
      p.process(sc.block);
      for (let c = 0; c < nOut; ++c) { const o = p.getOutputBufferData(c); for (let j = 0; j < sc.block; ++j) outs[c][b * sc.block + j] = o[j]; }
      for (const f of sc.ffts) ring[f.id].write(sc.block);
      if ((b + 1) % every === 0) {
        p.processQueuedEvents((batch) => {
          for (const e of batch) {
            if (e.type === 'meter') { events.push({ type: 'meter', block: b, source: e.event.source === undefined ? null : e.event.source }); continue; }
            if (e.type !== 'fft') throw new Error('unexpected event ' + e.type);
            const src = e.event.source === undefined ? null : e.event.source;
            const f = sc.ffts.find(q => nameOf[q.id] === src);   // (the fft nodes of a scenario carry different names)
            if (!f) throw new Error(sc.name + ': event from an unknown node');
            const size = sizeOf[f.id], at = ring[f.id].read(size);
            if (at < 0) throw new Error(sc.name + ': the ring replay says this node had nothing to hand on at block ' + b);
            if (e.event.data.real.length !== size / 2 + 1 || e.event.data.imag.length !== size / 2 + 1) throw new Error('bin count');
            events.push({ type: 'fft', block: b, source: src, size, frame: at, re: Float32Array.from(e.event.data.real), im: Float32Array.from(e.event.data.imag) });
          }
        });
      }
      for (const ch of (sc.changes || [])) if (ch.after_block === b) {
        r = p.postMessageBatch([[3, ch.id, ch.key, ch.value], [5]]);
        if (!r.success) throw new Error(r.message);
        sizeOf[ch.id] = ch.value;
      }
    }
    // outputs: the stored head, the rest must be the input itself
    for (let c = 0; c < nOut; ++c) for (let j = OUT_STORED; j < total; ++j) if (outs[c][j] !== x[j]) throw new Error(sc.name + ': output differs from the input after the fade at frame ' + j);
    const m = { graph: sc.graph, block: sc.block, blocks: sc.blocks, relay_every: every, ffts: sc.ffts, meter: sc.meter || null, changes: sc.changes || [],
                out_channels: nOut, out_offsets: [], events: [] };
    for (let c = 0; c < nOut; ++c) m.out_offsets.push(push(outs[c].slice(0, OUT_STORED)));
    const nFft = events.filter(e => e.type === 'fft').length;
    let k = 0;
    for (const e of events) {
      if (e.type === 'meter') { m.events.push({ type: 'meter', block: e.block, source: e.source }); continue; }
      // the frame the node transformed, and the reference's own error against a float64 DFT of it
      const w = windowOf(e.size), frame = new Float64Array(e.size);
      for (let i = 0; i < e.size; ++i) frame[i] = Math.fround((e.frame + i < 0 ? 0.0 : x[e.frame + i]) * w[i]);
      const d = dft(frame);
      let err = 0.0, peak = 0.0;
      for (let q = 0; q <= e.size / 2; ++q) {
        err = Math.max(err, Math.abs(e.re[q] - d.re[q]), Math.abs(e.im[q] - d.im[q]));
        peak = Math.max(peak, Math.abs(d.re[q]), Math.abs(d.im[q]));
      }
      if (!(err < 1e-4)) throw new Error(sc.name + ': event at block ' + e.block + ' is not the transform of the frame the ring replay names (' + err + ')');
      manifest.E_ref[e.size] = Math.max(manifest.E_ref[e.size] || 0.0, err);
      manifest.peak[e.size] = Math.max(manifest.peak[e.size] || 0.0, peak);
      const rec = { type: 'fft', block: e.block, source: e.source, size: e.size, frame: e.frame, offset: null };
      if (sc.store(k, nFft)) { rec.offset = push(e.re); push(e.im); }
      m.events.push(rec);
      ++k;
    }
    manifest.scenarios[sc.name] = m;
    p.delete();
  }
  // (j) rejected property values: the result of the batch that sets them, and that the earlier size stays in force
  {
    const p = new M.ElementaryAudioProcessor(1, 1);
    p.prepare(48000, 512);
    let r = p.postMessageBatch(batchOf({ graph: 'single', ffts: [{ id: 2, props: { size: 512 } }] }));
    if (!r.success) throw new Error(r.message);
    const tries = [['size', 300], ['size', 128], ['size', 16384], ['size', 'big'], ['size', 8192], ['size', 512], ['name', 5], ['name', 'ok']];
    for (const t of tries) {
      r = p.postMessageBatch([[3, 2, t[0], t[1]], [5]]);
      manifest.rejected.push({ key: t[0], value: t[1], success: !!r.success, message: r.message });
    }
    // size 512, then a rejected 300: still one event per 512-frame block
    r = p.postMessageBatch([[3, 2, 'size', 300], [5]]);
    let count = 0, bins = 0;
    for (let b = 0; b < 4; ++b) { p.process(512); p.processQueuedEvents((batch) => { for (const e of batch) if (e.type === 'fft') { ++count; bins = e.event.data.real.length; } }); }
    manifest.rejected_keeps = { size_before: 512, rejected: 300, blocks: 4, events: count, bins };
    p.delete();
  }
  fs.writeFileSync(path.join(HERE, 'fft_wasm.f32'), Buffer.concat(chunks));
  fs.writeFileSync(path.join(HERE, 'fft_wasm.json'), JSON.stringify(manifest, null, 1));
  console.log('floats', offset, 'E_ref', manifest.E_ref, 'peak', manifest.peak);
  for (const n of Object.keys(manifest.scenarios)) console.log(n, manifest.scenarios[n].events.filter(e => e.type === 'fft').map(e => e.block).join(','));
  console.log(manifest.rejected, manifest.rejected_keeps);
})().catch(e => { console.error(e); process.exit(1); });
