// TEST INFRASTRUCTURE: plays a .gtm file through the reference's own browser player and prints what it drew.
//
//   node ref_player.js <dir holding lzma.js, lzma.shim.js and gtm.player.js> <file.gtm>
//
// The three scripts are read from the reference tree at run time and evaluated in one fresh context, in the order
// the reference's index.html loads them; nothing of them is stored anywhere.  Everything below is ours: a canvas
// that starts opaque black (what fillRect with 'black' leaves, the colour of positions the player never draws),
// timers that never fire -- the frames are stepped from here -- and a console that keeps the error lines.
//
// One JSON object on stdout:
//   frames        frames played in the first pass over the file (up to the player's loop point)
//   width, height the tilemap's size in tiles
//   frame_sha256  per frame, SHA-256 of the RGBA framebuffer bytes (row-major, R,G,B,A) after that frame
//   clip_sha256   SHA-256 of all those framebuffers end to end
//   stalls        decodeFrame calls that drew nothing (the player waiting for its bandwidth-limited LZMA decode)
//   errors        every console.error line, and an exception or a runaway wait if one ended the run
// Written for node 12.
'use strict';

const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const vm = require('vm');

const MAX_STALLS = 1000000; // consecutive calls without a frame: the decoder makes no progress

function blackImage(w, h) {
  const data = new Uint8ClampedArray(w * h * 4);
  for (let i = 3; i < data.length; i += 4) data[i] = 255;
  return { width: w, height: h, data: data };
}

function main(dir, file) {
  const errors = [];
  const canvas = { // index.html's <canvas id="frame" width="8" height="8">
    width: 8,
    height: 8,
    getContext: function () {
      return {
        fillStyle: '',
        fillRect: function () {},
        putImageData: function () {},
        getImageData: function (x, y, w, h) { return blackImage(w, h); },
      };
    },
  };
  const sandbox = {
    document: { getElementById: function () { return canvas; } },
    setTimeout: function () { return 0; },
    setInterval: function () { return 0; },
    console: {
      log: function () {},
      warn: function () {},
      error: function () { errors.push(Array.prototype.map.call(arguments, String).join(' ').trim()); },
    },
  };
  vm.createContext(sandbox);
  ['lzma.js', 'lzma.shim.js', 'gtm.player.js'].forEach(function (name) {
    const p = path.join(dir, name);
    vm.runInContext(fs.readFileSync(p, 'utf8'), sandbox, { filename: p });
  });

  const bytes = fs.readFileSync(file);
  const input = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.length);
  const digests = [];
  const clip = crypto.createHash('sha256');
  let stalls = 0;
  try {
    sandbox.gtmCanvasId = 'frame';
    sandbox.gtmInStream = new sandbox.LZMA.iStream(input);
    sandbox.startFromReader();
    let waiting = 0;
    while (sandbox.gtmLoopCount < 1) {
      const at = sandbox.gtmDataPos;
      sandbox.decodeFrame();
      // a call that read commands moved the read position, or wrapped it to 0 and counted a loop
      if (sandbox.gtmDataPos === at && sandbox.gtmLoopCount < 1) {
        stalls++;
        if (++waiting > MAX_STALLS) throw new Error('no frame after ' + MAX_STALLS + ' calls');
        continue;
      }
      waiting = 0;
      const d = sandbox.gtmTMImageData.data;
      const frame = Buffer.from(d.buffer, d.byteOffset, d.byteLength);
      digests.push(crypto.createHash('sha256').update(frame).digest('hex'));
      clip.update(frame);
    }
  } catch (e) {
    errors.push('exception: ' + (e && e.message ? e.message : String(e)));
  }
  process.stdout.write(JSON.stringify({
    frames: digests.length,
    width: sandbox.gtmWidth,
    height: sandbox.gtmHeight,
    frame_sha256: digests,
    clip_sha256: clip.digest('hex'),
    stalls: stalls,
    errors: errors,
  }) + '\n');
}

if (process.argv.length !== 4) {
  process.stderr.write('usage: node ref_player.js <reference decoders/htmljs dir> <file.gtm>\n');
  process.exit(2);
}
main(process.argv[2], process.argv[3]);
