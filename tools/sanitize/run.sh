#!/bin/bash
# Host code of the JPEG stages under AddressSanitizer + UndefinedBehaviorSanitizer (no GPU): the file writer on random
# coefficient planes with every option, and the header parser + un-stuffing + decode-table builders + host walkers
# (ifhip_jpeg_debug_scan_report) on mutated copies of committed files; the WebP decoder's container walk, prepare and token loop
# on mutated copies of the tests' files; the GIF decoder's container walk and the whole batch on the CPU, likewise; the querystring parser and layout behind command_string on damaged strings.
# Builds into /tmp; prints one summary line each.
set -eu
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
W=/tmp/ifhip_sanitize; rm -rf $W; mkdir -p $W; cd $W
INC="-I$ROOT/imageflow_amd/csrc -I$ROOT/include"
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17"
g++ $SAN $INC -o writer_fuzz "$ROOT/tools/sanitize/writer_fuzz.cpp" "$ROOT/imageflow_amd/csrc/jpeg_write.cpp" "$ROOT/tools/sanitize/stubs.cpp"
./writer_fuzz
# the JPEG front end (marker walk, parser, un-stuffing, EXIF, ICC) and the entropy stage's host half (decode tables, host
# walkers of the scan report): plain host code, one g++ line
g++ $SAN $INC -c "$ROOT/imageflow_amd/csrc/jpeg_parse.cpp" -o jpeg_parse.o
g++ $SAN -c "$ROOT/tools/sanitize/stubs.cpp" -o stubs.o
g++ $SAN $INC -o parser_fuzz "$ROOT/tools/sanitize/parser_fuzz.cpp" jpeg_parse.o "$ROOT/imageflow_amd/csrc/jpeg_entropy_tables.cpp" "$ROOT/imageflow_amd/csrc/jpeg_scan_report.cpp" stubs.o
python3 - "$ROOT" <<'PY'
import sys, numpy as np
z = np.load(sys.argv[1] + "/tests/golden/jpeg_entropy_cases.npz")
for i in (0, 5, 17, 33, 48, 60):
    open(f"/tmp/ifhip_sanitize/case_{i}.jpg", "wb").write(z[f"jpg_{i}"].tobytes())
PY
ASAN_OPTIONS=detect_leaks=0 ./parser_fuzz case_*.jpg
# the WebP decoder's host side: container walk, prepare and the token loop on mutated copies of the tests' files
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --cuda-host-only $SAN $INC -c "$ROOT/imageflow_amd/csrc/webp_read.cpp" -o webp_read_host.o 2>/dev/null
g++ $SAN -fno-sanitize=vptr $INC -c "$ROOT/tools/sanitize/webp_fuzz.cpp" -o webp_fuzz.o      # (vptr: g++ and the clang runtime that links disagree on it)
/opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined -o webp_fuzz webp_fuzz.o webp_read_host.o jpeg_parse.o stubs.o -lpthread
(cd "$ROOT" && python3 - <<'PY'
from tests import webp_decode_fixtures as X
files = X.good_files()
for name in ("photo_q100_m6", "photo_cache", "indexed_16", "graphic", "own_two_bands", "gen_predictor_after_indexing", "gen_tile_bits_9_cache_11", "gen_meta_groups",
             "gen_codes", "gen_simple_code_symbol_beyond_the_alphabet", "gen_vp8x_wrapped"):
    open("/tmp/ifhip_sanitize/case_%s.webp" % name, "wb").write(files[name])
for name, (data, _) in X.damaged_files().items():
    open("/tmp/ifhip_sanitize/case_bad_%s.webp" % name, "wb").write(data)
PY
)
ASAN_OPTIONS=detect_leaks=0 ./webp_fuzz case_*.webp
# the GIF decoder: container walk and the whole batch as the device runs it (plain host code, no HIP) on mutated copies of the tests' files
g++ $SAN $INC -o gif_fuzz "$ROOT/tools/sanitize/gif_fuzz.cpp" "$ROOT/imageflow_amd/csrc/gif_read.cpp" "$ROOT/tools/sanitize/stubs.cpp"
(cd "$ROOT" && python3 - <<'PY'
from tests import gif_fixtures as X
good = X.good_files()
for name in ("m1_noise", "m8_runs", "widths_m2_clear_at_full", "deferred_m8_long_tail", "clear_at_64", "mixed_segments", "flat_kwkwk_chain", "interlaced_h9",
             "dispose_previous_frame2", "dispose_mixed_frame2", "zero_size_frame_then_one", "gif87a_with_extensions", "no_global_palette"):
    open("/tmp/ifhip_sanitize/case_%s.gif" % name, "wb").write(good[name][0])
for name, (data, _, _) in X.damaged_files().items():
    open("/tmp/ifhip_sanitize/case_bad_%s.gif" % name, "wb").write(data)
for name, data in X.golden_files().items():
    open("/tmp/ifhip_sanitize/case_golden_%s" % name, "wb").write(data)
PY
)
ASAN_OPTIONS=detect_leaks=0 ./gif_fuzz case_*.gif
# the querystring layer (Instructions parser, colour reader, Ir4Layout, watermark splitter): untrusted text, plain host code
g++ $SAN $INC -o querystring_fuzz "$ROOT/tools/sanitize/querystring_fuzz.cpp" "$ROOT/imageflow_amd/csrc/querystring.cpp" "$ROOT/imageflow_amd/csrc/layout.cpp" "$ROOT/tools/sanitize/stubs.cpp"
./querystring_fuzz
# encoder selection (the querystring's output keys, serde's readers of the presets `auto` / `format`, the quality tables and the resolution): plain host code
g++ $SAN -ffp-contract=off $INC -o encoder_select_fuzz "$ROOT/tools/sanitize/encoder_select_fuzz.cpp" "$ROOT/imageflow_amd/csrc/encoder_select.cpp" "$ROOT/imageflow_amd/csrc/querystring.cpp" \
  "$ROOT/imageflow_amd/csrc/layout.cpp" "$ROOT/imageflow_amd/csrc/shim_json.cpp" "$ROOT/tools/sanitize/stubs.cpp"
./encoder_select_fuzz
# the whole library host-only (every translation unit, device blobs replaced by empty stand-ins) behind the libimageflow
# ABI subset: damaged JSON jobs
mkdir -p lib && : > fatbin_stubs.c
OBJS=""
for src in "$ROOT"/imageflow_amd/csrc/*.cpp "$ROOT"/imageflow_amd/csrc/*.hip; do
  base=$(basename "$src")
  if [ "$base" = "resample_fused.hip" ]; then
    for k in 1 2 3 4 5 6 7 8; do
      /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --cuda-host-only $SAN $INC -DIFHIP_FUSED_K=$k -c "$src" -o lib/fused_$k.o 2>/dev/null &
      OBJS="$OBJS lib/fused_$k.o"
    done
  elif [ "$base" = "resample_ws.hip" ]; then
    for k in 1 2 3 4 5; do
      /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --cuda-host-only $SAN $INC -DIFHIP_FUSED_K=$k -c "$src" -o lib/ws_$k.o 2>/dev/null &
      OBJS="$OBJS lib/ws_$k.o"
    done
  else
    /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --cuda-host-only $SAN $INC -c "$src" -o lib/$base.o 2>/dev/null &
    OBJS="$OBJS lib/$base.o"
  fi
done
wait
for o in $OBJS; do
  for sym in $(nm $o | awk '/ U __hip_fatbin_/ {print $2}'); do printf '__attribute__((section(".hip_fatbin"))) const char %s[64] = {0};\n' "$sym" >> fatbin_stubs.c; done
done
sort -u fatbin_stubs.c -o fatbin_stubs.c
gcc -c fatbin_stubs.c -o fatbin_stubs.o
g++ $SAN $INC -c "$ROOT/tools/sanitize/json_fuzz.cpp" -o json_fuzz.o
/opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined -o json_fuzz json_fuzz.o $OBJS fatbin_stubs.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lpthread
ASAN_OPTIONS=detect_leaks=0 ./json_fuzz
