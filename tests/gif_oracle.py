"""The GIF reader's yardstick in plain Python: a serial LZW decoder, the container walk, and Screen::blit / Disposal of the
reference (imageflow_core/src/codecs/gif/{screen,disposal}.rs) pixel by pixel.  tests/test_gif_oracle.py pins the LZW
decoder to Pillow's indices on Pillow-written files and the compositing to hand-checked cases.

Status words are those of include/imageflow_hip.h (IFHIP_GIF_DEC_*)."""
import struct

import numpy as np

OK, TOO_LITTLE, BAD_CODE, CONTAINER, MIN_CODE_SIZE, NO_PALETTE, FRAME_TOO_LARGE, NO_SUCH_FRAME = range(8)
ANY, KEEP, BACKGROUND, PREVIOUS = 0, 1, 2, 3


def lzw_decode(stream, m, want):
    """-> (status, indices): the first `want` indices of the stream; what lies behind them is ignored."""
    clear, end = 1 << m, (1 << m) + 1
    out = bytearray()
    prefix, suffix = {}, {}
    size, width, prev = clear + 2, m + 1, None
    pos, nbits = 0, len(stream) * 8
    acc = int.from_bytes(stream, "little")

    def string(c):
        s = bytearray()
        while c >= clear:
            s.append(suffix[c])
            c = prefix[c]
        s.append(c)
        return s[::-1]

    while True:
        width = m + 1
        while prev is not None and width < 12 and size >= (1 << width):
            width += 1
        if pos + width > nbits:
            break
        c = (acc >> pos) & ((1 << width) - 1)
        pos += width
        if c == clear:
            prefix, suffix = {}, {}
            size, width, prev = clear + 2, m + 1, None
            continue
        if c == end:
            break
        if prev is None:
            if c >= clear:
                return BAD_CODE, None
            out.append(c)
        else:
            if c < size:
                s = string(c)
            elif c == size and size < 4096:
                s = string(prev)
                s.append(s[0])
            else:
                return BAD_CODE, None
            if size < 4096:
                prefix[size], suffix[size] = prev, s[0]
                size += 1
            out += s
        prev = c                                           # (the rest of the stream is still validated, as the device does)
    if len(out) < want:
        return TOO_LITTLE, None
    return OK, np.frombuffer(bytes(out[:want]), np.uint8)


def parse(data, target=0):
    """The container up to frame `target`.  -> dict(status, w, h, bg, global_palette, frames, frames_seen)"""
    d = bytes(data)
    if len(d) < 13 or d[:6] not in (b"GIF87a", b"GIF89a"):
        return None
    w, h, flags, bgi, _ = struct.unpack("<HHBBB", d[6:13])
    out = dict(status=OK, w=w, h=h, bg=(0, 0, 0, 0), global_palette=None, frames=[], frames_seen=0)
    pos = 13
    if flags & 0x80:
        n = 2 << (flags & 7)
        if pos + 3 * n > len(d):
            out["status"] = CONTAINER
            return out
        out["global_palette"] = np.frombuffer(d[pos:pos + 3 * n], np.uint8).reshape(n, 3)
        pos += 3 * n
        if bgi < n:
            r, g, b = out["global_palette"][bgi]
            out["bg"] = (int(b), int(g), int(r), 255)
    gce = None

    def skip_blocks(p):
        while True:
            if p >= len(d):
                return None
            n = d[p]
            p += 1
            if n == 0:
                return p
            p += n

    while len(out["frames"]) <= target:
        if pos >= len(d) or d[pos] == 0x3B:
            break
        kind = d[pos]
        pos += 1
        if kind == 0x21:
            if pos >= len(d):
                break
            label = d[pos]
            pos += 1
            if label == 0xF9 and pos < len(d) and d[pos] == 4 and pos + 5 <= len(d):
                f, delay, tr = struct.unpack("<BHB", d[pos + 1:pos + 5])
                dispose = (f >> 2) & 7
                gce = dict(dispose=dispose if dispose <= 3 else KEEP, transparent=tr if f & 1 else None, delay=delay, user_input=bool(f & 2))
            pos = skip_blocks(pos)
            if pos is None:
                break
        elif kind == 0x2C:
            if pos + 9 > len(d):
                break
            left, top, fw, fh, ff = struct.unpack("<HHHHB", d[pos:pos + 9])
            pos += 9
            fr = dict(left=left, top=top, w=fw, h=fh, interlace=bool(ff & 0x40), palette=None, dispose=KEEP, transparent=None, delay=0, user_input=False)
            if gce:
                fr.update(gce)
            gce = None
            if ff & 0x80:
                n = 2 << (ff & 7)
                if pos + 3 * n > len(d):
                    break
                fr["palette"] = np.frombuffer(d[pos:pos + 3 * n], np.uint8).reshape(n, 3)
                pos += 3 * n
            if pos >= len(d):
                break
            fr["m"] = d[pos]
            pos += 1
            stream = bytearray()
            while pos < len(d) and d[pos]:
                stream += d[pos + 1:pos + 1 + d[pos]]
                pos += 1 + d[pos]
            pos = min(pos + 1, len(d)) if pos < len(d) else len(d)
            fr["stream"] = bytes(stream)
            out["frames"].append(fr)
            out["frames_seen"] += 1
            if not 1 <= fr["m"] <= 8:
                out["status"] = MIN_CODE_SIZE
                return out
            if fw * fh > 16 * 1024 * 1024:
                out["status"] = FRAME_TOO_LARGE
                return out
            if fr["palette"] is None and out["global_palette"] is None:
                out["status"] = NO_PALETTE
                return out
        else:
            out["status"] = CONTAINER
            return out
    if len(out["frames"]) <= target:
        out["status"] = NO_SUCH_FRAME
    return out


def row_map(h):
    return [y for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(start, h, step)]


def frame_indices(fr):
    """-> (status, [h, w] indices in image order)"""
    st, idx = lzw_decode(fr["stream"], fr["m"], fr["w"] * fr["h"])
    if st:
        return st, None
    idx = idx.reshape(fr["h"], fr["w"])
    if fr["interlace"] and fr["h"]:
        out = np.empty_like(idx)
        out[row_map(fr["h"])] = idx
        idx = out
    return OK, idx


def compose(P, target):
    """Screen::new, then blit for frames 0..target -> BGRA [h, w, 4]"""
    W, H = P["w"], P["h"]
    screen = np.empty((H, W, 4), np.uint8)
    screen[:] = P["bg"]
    prev = None                                            # (method, l, t, w, h, saved)
    for fr in P["frames"][:target + 1]:
        pal = fr["palette"] if fr["palette"] is not None else P["global_palette"]
        left, top = min(fr["left"], W), min(fr["top"], H)
        sw, sh = min(fr["w"], W - left), min(fr["h"], H - top)
        if prev is not None and prev[3] and prev[4]:
            method, l, t, w, h, saved = prev
            if method == BACKGROUND:
                screen[t:t + h, l:l + w] = P["bg"]
            elif method == PREVIOUS:
                screen[t:t + h, l:l + w] = saved
        saved = screen[top:top + sh, left:left + sw].copy() if fr["dispose"] == PREVIOUS and sw and sh else None
        prev = (fr["dispose"], left, top, sw, sh, saved)
        if not sw or not sh:
            continue
        st, idx = frame_indices(fr)
        assert st == OK
        for y in range(sh):
            for x in range(sw):
                i = int(idx[y, x])
                if fr["transparent"] is not None and i == fr["transparent"]:
                    continue
                if i < len(pal):
                    r, g, b = pal[i]
                    screen[top + y, left + x] = (b, g, r, 255)
                else:
                    screen[top + y, left + x] = (0, 0, 0, 0)
    return screen


def decode(data, target=0):
    """-> (status, BGRA [h, w, 4] or None, parsed)"""
    P = parse(data, target)
    if P is None or not P["w"] or not P["h"]:                 # no header, or a logical screen without pixels: no canvas to decode into
        return CONTAINER, None, P
    if P["status"]:
        return P["status"], None, P
    for fr in P["frames"]:
        st, _ = frame_indices(fr)
        if st:
            return st, None, P
    return OK, compose(P, target), P
