"""Instructions::delete_from_map (imageflow_riapi/src/ir4/parsing.rs:481-635) with the Parser helpers (:692-1103) and the colour
helpers (imageflow_helpers/src/colors.rs:36-75).  -> a dict that holds only the keys that parsed.

Where this library departs from the reference, so does this file, and says so: a key outside the list below is refused
(the reference warns), `autorotate=false` is refused, an unknown filter name is an error, a repeated key counts once (the
last), `width` / `height` read a non-integer the way C's strtod does, `format` is jpg | jpeg or refused."""
import math
import re

import numpy as np


class Refused(Exception):
    """ActionNotSupported: a key or value this library does not honour"""


class Invalid(Exception):
    """InvalidNodeParams: an unknown filter name, a size beyond an i32"""


class NotModelled(Exception):
    """the reference panics or overflows here; callers that draw random strings draw again"""


KEYS = {"width", "w", "height", "h", "maxwidth", "maxheight", "zoom", "dpr", "dppx", "mode", "stretch", "crop", "scale", "cropxunits",
        "cropyunits", "c", "c.gravity", "anchor", "srotate", "rotate", "sflip", "sourceflip", "flip", "bgcolor", "s.alpha", "s.brightness",
        "s.contrast", "s.saturation", "s.sepia", "s.grayscale", "f.sharpen", "f.sharpen_when", "up.filter", "down.filter", "up.colorspace",
        "down.colorspace", "watermark_red_dot", "ignoreicc", "decoder.min_precise_scaling_ratio", "autorotate", "quality", "jpeg.quality",
        "format", "s.roundcorners", "a.balancewhite", "trim.threshold", "trim.percentpadding"}
WS = " \t\r\n\f\v"
_FLOAT = re.compile(r"[+-]?(?:inf|infinity|nan|(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?)\Z", re.I)       # str::parse::<f64>
_INT = re.compile(r"[+-]?\d+\Z")
_STRTOD = re.compile(r"\s*[+-]?(?:inf(?:inity)?|nan|(?P<hex>0x(?:[0-9a-f]+\.?[0-9a-f]*|\.[0-9a-f]+)(?:p[+-]?\d+)?)|(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?)", re.I)
FILTERS = ["robidoux_fast", "robidoux", "robidoux_sharp", "ginseng", "ginseng_sharp", "lanczos", "lanczos_sharp", "lanczos_2", "lanczos_2_sharp",
           "cubic", "cubic_sharp", "catmull_rom", "mitchell", "cubic_b_spline", "hermite", "jinc", "triangle", "linear", "box", "fastest",
           "n_cubic", "n_cubic_sharp"]
CSS = {
    "aliceblue": 0xFFF0F8FF, "antiquewhite": 0xFFFAEBD7, "aqua": 0xFF00FFFF, "aquamarine": 0xFF7FFFD4, "azure": 0xFFF0FFFF, "beige": 0xFFF5F5DC,
    "bisque": 0xFFFFE4C4, "black": 0xFF000000, "blanchedalmond": 0xFFFFEBCD, "blue": 0xFF0000FF, "blueviolet": 0xFF8A2BE2, "brown": 0xFFA52A2A,
    "burlywood": 0xFFDEB887, "cadetblue": 0xFF5F9EA0, "chartreuse": 0xFF7FFF00, "chocolate": 0xFFD2691E, "coral": 0xFFFF7F50,
    "cornflowerblue": 0xFF6495ED, "cornsilk": 0xFFFFF8DC, "crimson": 0xFFDC143C, "cyan": 0xFF00FFFF, "darkblue": 0xFF00008B, "darkcyan": 0xFF008B8B,
    "darkgoldenrod": 0xFFB8860B, "darkgray": 0xFFA9A9A9, "darkgreen": 0xFF006400, "darkgrey": 0xFFA9A9A9, "darkkhaki": 0xFFBDB76B,
    "darkmagenta": 0xFF8B008B, "darkolivegreen": 0xFF556B2F, "darkorange": 0xFFFF8C00, "darkorchid": 0xFF9932CC, "darkred": 0xFF8B0000,
    "darksalmon": 0xFFE9967A, "darkseagreen": 0xFF8FBC8F, "darkslateblue": 0xFF483D8B, "darkslategray": 0xFF2F4F4F, "darkslategrey": 0xFF2F4F4F,
    "darkturquoise": 0xFF00CED1, "darkviolet": 0xFF9400D3, "deeppink": 0xFFFF1493, "deepskyblue": 0xFF00BFFF, "dimgray": 0xFF696969,
    "dimgrey": 0xFF696969, "dodgerblue": 0xFF1E90FF, "firebrick": 0xFFB22222, "floralwhite": 0xFFFFFAF0, "forestgreen": 0xFF228B22,
    "fuchsia": 0xFFFF00FF, "gainsboro": 0xFFDCDCDC, "ghostwhite": 0xFFF8F8FF, "gold": 0xFFFFD700, "goldenrod": 0xFFDAA520, "gray": 0xFF808080,
    "green": 0xFF008000, "greenyellow": 0xFFADFF2F, "grey": 0xFF808080, "honeydew": 0xFFF0FFF0, "hotpink": 0xFFFF69B4, "indianred": 0xFFCD5C5C,
    "indigo": 0xFF4B0082, "ivory": 0xFFFFFFF0, "khaki": 0xFFF0E68C, "lavender": 0xFFE6E6FA, "lavenderblush": 0xFFFFF0F5, "lawngreen": 0xFF7CFC00,
    "lemonchiffon": 0xFFFFFACD, "lightblue": 0xFFADD8E6, "lightcoral": 0xFFF08080, "lightcyan": 0xFFE0FFFF, "lightgoldenrodyellow": 0xFFFAFAD2,
    "lightgray": 0xFFD3D3D3, "lightgreen": 0xFF90EE90, "lightgrey": 0xFFD3D3D3, "lightpink": 0xFFFFB6C1, "lightsalmon": 0xFFFFA07A,
    "lightseagreen": 0xFF20B2AA, "lightskyblue": 0xFF87CEFA, "lightslategray": 0xFF778899, "lightslategrey": 0xFF778899,
    "lightsteelblue": 0xFFB0C4DE, "lightyellow": 0xFFFFFFE0, "lime": 0xFF00FF00, "limegreen": 0xFF32CD32, "linen": 0xFFFAF0E6, "magenta": 0xFFFF00FF,
    "maroon": 0xFF800000, "mediumaquamarine": 0xFF66CDAA, "mediumblue": 0xFF0000CD, "mediumorchid": 0xFFBA55D3, "mediumpurple": 0xFF9370DB,
    "mediumseagreen": 0xFF3CB371, "mediumslateblue": 0xFF7B68EE, "mediumspringgreen": 0xFF00FA9A, "mediumturquoise": 0xFF48D1CC,
    "mediumvioletred": 0xFFC71585, "midnightblue": 0xFF191970, "mintcream": 0xFFF5FFFA, "mistyrose": 0xFFFFE4E1, "moccasin": 0xFFFFE4B5,
    "navajowhite": 0xFFFFDEAD, "navy": 0xFF000080, "oldlace": 0xFFFDF5E6, "olive": 0xFF808000, "olivedrab": 0xFF6B8E23, "orange": 0xFFFFA500,
    "orangered": 0xFFFF4500, "orchid": 0xFFDA70D6, "palegoldenrod": 0xFFEEE8AA, "palegreen": 0xFF98FB98, "paleturquoise": 0xFFAFEEEE,
    "palevioletred": 0xFFDB7093, "papayawhip": 0xFFFFEFD5, "peachpuff": 0xFFFFDAB9, "peru": 0xFFCD853F, "pink": 0xFFFFC0CB, "plum": 0xFFDDA0DD,
    "powderblue": 0xFFB0E0E6, "purple": 0xFF800080, "rebeccapurple": 0xFF663399, "red": 0xFFFF0000, "rosybrown": 0xFFBC8F8F, "royalblue": 0xFF4169E1,
    "saddlebrown": 0xFF8B4513, "salmon": 0xFFFA8072, "sandybrown": 0xFFF4A460, "seagreen": 0xFF2E8B57, "seashell": 0xFFFFF5EE, "sienna": 0xFFA0522D,
    "silver": 0xFFC0C0C0, "skyblue": 0xFF87CEEB, "slateblue": 0xFF6A5ACD, "slategray": 0xFF708090, "slategrey": 0xFF708090, "snow": 0xFFFFFAFA,
    "springgreen": 0xFF00FF7F, "steelblue": 0xFF4682B4, "tan": 0xFFD2B48C, "teal": 0xFF008080, "thistle": 0xFFD8BFD8, "tomato": 0xFFFF6347,
    "turquoise": 0xFF40E0D0, "violet": 0xFFEE82EE, "wheat": 0xFFF5DEB3, "white": 0xFFFFFFFF, "whitesmoke": 0xFFF5F5F5, "yellow": 0xFFFFFF00,
    "yellowgreen": 0xFF9ACD32,
    "transparent": 0}


def form_decode(s):
    """application/x-www-form-urlencoded as Url::query_pairs reads it, on bytes kept as latin-1 characters"""
    out, i = [], 0
    while i < len(s):
        if s[i] == "+":
            out.append(" ")
        elif s[i] == "%" and re.match(r"[0-9a-fA-F]{2}", s[i + 1:i + 3]):
            out.append(chr(int(s[i + 1:i + 3], 16)))
            i += 2
        else:
            out.append(s[i])
        i += 1
    return "".join(out)


def f64(s):
    return float(s) if _FLOAT.match(s) else None


def f32(s, finite=True):
    if not _FLOAT.match(s):
        return None
    with np.errstate(over="ignore"):
        v = np.float32(float(s))
    return None if finite and not np.isfinite(v) else v


def i32(s):
    if not _INT.match(s):
        return None
    v = int(s)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def boolean(s):
    s = s.lower()
    return True if s in ("true", "1", "yes", "on") else False if s in ("false", "0", "no", "off") else None


def f64_list(s, n, lenient=False):
    parts = [f64(p.strip(WS)) for p in s.split(",")]
    if lenient:
        parts = [0.0 if p is None else p for p in parts]
    return parts if len(parts) == n and None not in parts else None


def color(value):
    """parse_color_hex_or_named -> 0xAARRGGBB or None"""
    if any(ord(ch) >= 0x80 for ch in value):
        return None
    v = value[1:] if value[:1] == "#" else value
    if v.startswith("+"):
        raise NotModelled("u32::from_str_radix takes the '+', the slicing behind it panics or reads it as a digit")
    if not re.match(r"[0-9a-fA-F]+\Z", v) or int(v, 16) > 0xFFFFFFFF:
        return CSS.get(value.lower())
    if len(v) not in (3, 4, 6, 8):
        return None
    n = 1 if len(v) < 6 else 2
    ch = [v[k:k + n] * (3 - n) for k in range(0, len(v), n)] + ["ff"] * (len(v) in (3, 6))
    r, g, b, a = (int(c, 16) for c in ch)
    return a << 24 | r << 16 | g << 8 | b


def filter_name(v):
    want = v.replace("_", "").lower()
    for n in FILTERS:
        if n.replace("_", "") == want:
            return n
    raise Invalid("filter " + v)


def side(raw):
    t = raw.strip(WS)
    if not t:
        return None
    v = i32(t)
    if v is not None:
        return v
    m = _STRTOD.match(raw)
    d = 0.0 if not m else float.fromhex(m.group(0).strip()) if m.group("hex") else float(m.group(0))
    if not (0 <= d <= 2147483647.0):
        raise Invalid("width/height out of range")
    return int(d) if d >= 1 else None


def parse(text):
    if "#" in text:
        raise Refused("#")
    i, m = {}, {}
    for kv in text.split("&"):
        if "=" not in kv:
            continue
        k, v = kv.split("=", 1)
        k, v = "".join(c.lower() if c < "\x80" else c for c in form_decode(k)), form_decode(v)
        if k not in KEYS:
            raise Refused(k)
        if k in ("down.filter", "up.filter"):
            i[k.replace(".", "_")] = filter_name(v)
        elif k in ("quality", "jpeg.quality"):
            if re.match(r"\s*[+-]?\d+\Z", v):
                i[k.replace(".", "_")] = max(0, min(100, int(v)))
            else:
                i["jpeg_out"] = True
        elif k == "format":
            if v.lower() not in ("jpg", "jpeg"):
                raise Refused("format=" + v)
            i["jpeg_out"] = i["format_jpeg"] = True
        elif k == "s.roundcorners":
            s = v.strip(WS)
            vals = (f64_list(s, 4) or (f64_list(s, 1) or [])[:1] * 4) if s else None
            if vals:
                i["s_round_corners"] = vals
        elif k == "a.balancewhite":
            if v.strip(WS).lower() in ("true", "area"):
                i["a_balance_white"] = True
        elif k == "trim.threshold":
            if i32(v.strip(WS)) is not None:
                i["trim_threshold"] = i32(v.strip(WS))
        elif k == "trim.percentpadding":
            if f32(v.strip(WS)) is not None:
                i["trim_padding"] = f32(v.strip(WS))
        else:
            m[k] = v.strip(WS)
    m = {k: v for k, v in m.items() if v}

    def put(name, value):
        if value is not None:
            i[name] = value

    def first(name, keys, fn):
        for k in keys:
            if name not in i and k in m:
                put(name, fn(m[k]))
    first("w", ("width", "w"), side)
    first("h", ("height", "h"), side)
    first("legacy_max_width", ("maxwidth",), side)
    first("legacy_max_height", ("maxheight",), side)
    first("zoom", ("zoom", "dpr", "dppx"), lambda s: f32(s.rstrip("x")))
    flips = {"none": (False, False), "h": (True, False), "x": (True, False), "v": (False, True), "y": (False, True), "both": (True, True),
             "xy": (True, True)}
    first("flip", ("flip",), lambda s: flips.get(s.lower()))
    first("sflip", ("sflip", "sourceflip"), lambda s: flips.get(s.lower()))

    def rotate(s):                                      # parse_rotate (:962-974): round to a quarter turn, 0..270
        v = f32(s, finite=False)
        if v is None:
            return None
        q = np.float32(v) / np.float32(90)
        if np.isnan(q) or np.isinf(q):
            return 0
        r = np.float32(math.copysign(math.floor(abs(float(q)) + 0.5), float(q)))           # f32::round: half away from zero
        return ((int(math.fmod(float(r), 4.0)) + 4) % 4) * 90
    first("srotate", ("srotate",), rotate)
    first("rotate", ("rotate",), rotate)
    first("autorotate", ("autorotate",), boolean)
    modes = {"max": "max", "pad": "pad", "crop": "crop", "stretch": "stretch", "carve": "stretch", "aspectcrop": "aspectcrop"}
    first("mode", ("mode",), lambda s: modes.get(s.lower()))
    if "mode" not in i and m.get("stretch", "").lower() == "fill":
        i["mode"] = "stretch"
    if m.get("crop", "").lower() == "auto":
        i.setdefault("mode", "crop")
        del m["crop"]
    scales = {"down": "down", "downscaleonly": "down", "up": "up", "upscaleonly": "up", "both": "both", "canvas": "canvas", "upscalecanvas": "canvas"}
    first("scale", ("scale",), lambda s: scales.get(s.lower()))
    first("ignoreicc", ("ignoreicc",), boolean)
    spaces = {"srgb", "linear", "gamma"}
    first("down_colorspace", ("down.colorspace",), lambda s: s.lower() if s.lower() in spaces else None)
    first("up_colorspace", ("up.colorspace",), lambda s: s.lower() if s.lower() in spaces else None)
    c = f64_list(m["c"], 4) if "c" in m else None
    if c is not None:
        i["crop"], i["cropxunits"], i["cropyunits"] = c, 100.0, 100.0
    else:
        if "crop" in m:
            put("crop", f64_list(m["crop"], 4) or f64_list(m["crop"].replace("(", "").replace(")", "").strip(WS), 4, lenient=True))
        for k in ("cropxunits", "cropyunits"):
            if k in m and f64(m[k]) is not None and math.isfinite(f64(m[k])):
                i[k] = f64(m[k])
    first("c_gravity", ("c.gravity",), lambda s: f64_list(s, 2))
    near, center, far = ("near", None), ("center", None), ("far", None)
    names = {"topleft": (near, near), "topcenter": (center, near), "topright": (far, near), "middleleft": (near, center),
             "middlecenter": (center, center), "middleright": (far, center), "bottomleft": (near, far), "bottomcenter": (center, far),
             "bottomright": (far, far)}

    def anchor(s):
        s = s.lower()
        if s in names:
            return names[s]
        g = f64_list(s, 2)
        with np.errstate(over="ignore"):
            return None if g is None else (("percent", np.float32(g[0])), ("percent", np.float32(g[1])))
    first("anchor", ("anchor",), anchor)
    gray = {"true": "grayscale_ntsc", "y": "grayscale_ntsc", "ntsc": "grayscale_ntsc", "ry": "grayscale_ry", "flat": "grayscale_flat",
            "bt709": "grayscale_bt709"}
    first("s_grayscale", ("s.grayscale",), lambda s: gray.get(s.lower()))
    for k in ("s.contrast", "s.alpha", "s.saturation", "s.brightness", "f.sharpen", "decoder.min_precise_scaling_ratio"):
        first(k.replace("decoder.", "").replace(".", "_"), (k,), f32)
    first("s_sepia", ("s.sepia",), boolean)
    when = {"downscaling": "downscaling", "sizediffers": "size_differs", "always": "always"}
    first("f_sharpen_when", ("f.sharpen_when",), lambda s: when.get(s.lower()))
    first("bgcolor", ("bgcolor",), color)
    first("watermark_red_dot", ("watermark_red_dot",), boolean)
    if i.get("autorotate") is False:
        raise Refused("autorotate=false")
    return i
