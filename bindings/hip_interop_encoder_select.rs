// hip_interop_encoder_select.rs -- the declarations of include/imageflow_hip_encoder_select.h (encoder selection for the
// presets `auto` and `format`, csrc/encoder_select.cpp), beside the generated hip_interop.rs: that file names exactly what
// include/imageflow_hip.h declares.  Host only: no stream, no context.
// For codecs/auto.rs (create_encoder_auto) and imageflow_riapi's ir4/encoder.rs (calculate_encoder_preset).
use std::os::raw::{c_char, c_int};

pub const IFHIP_SELECT_OK: c_int = 0;
pub const IFHIP_SELECT_REFUSED: c_int = 2;
pub const IFHIP_SELECT_INVALID: c_int = 3;
pub const IFHIP_SELECT_INVALID_JSON: c_int = 4;
pub const IFHIP_SELECT_SOURCE_NONE: c_int = 0;
pub const IFHIP_SELECT_SOURCE_JPEG: c_int = 1;
pub const IFHIP_SELECT_SOURCE_PNG: c_int = 2;
pub const IFHIP_SELECT_SOURCE_GIF: c_int = 3;
pub const IFHIP_SELECT_SOURCE_WEBP: c_int = 4;

#[link(name = "imageflow_hip")]
extern "C" {
    pub fn ifhip_shim_querystring_encoder_preset(value: *const c_char, out: *mut c_char, cap: usize, needed: *mut usize) -> c_int;
    pub fn ifhip_shim_resolve_encoder_preset(preset_json: *const c_char, len: usize, source_kind: c_int, source_lossless: c_int, source_frames: u32, alpha_meaningful: c_int, w: u32, h: u32, out: *mut c_char, cap: usize, needed: *mut usize) -> c_int;
}
