"""What the tests of the ABI shim's JSON reader send it: two real job bodies -- a `steps` chain and a `graph` -- that they mutate and
truncate, the bodies that are no JSON and the numbers outside its grammar:
tests/test_abi_shim.py sends them through the library, tests/test_shim_json.py through the reader alone under the host sanitizers."""

MUTATED_JOBS = [
    {"io": [{"io_id": 0, "direction": "in", "io": "placeholder"}, {"io_id": 1, "direction": "out", "io": "output_buffer"}],
     "framewise": {"steps": [{"decode": {"io_id": 0, "commands": [{"jpeg_downscale_hints": {"width": 800, "height": 600, "scale_luma_spatially": True,
                                                                                            "gamma_correct_for_srgb_during_spatial_luma_scaling": True}}]}},
                             {"resample_2d": {"w": 200, "h": 200, "hints": {"down_filter": "robidoux", "scaling_colorspace": "linear", "sharpen_percent": 15,
                                                                              "background_color": {"srgb": {"hex": "FFFFFFFF"}}}}},
                             {"encode": {"io_id": 1, "preset": {"libjpeg_turbo": {"quality": 90, "progressive": True}}}}]}},
    {"framewise": {"graph": {"nodes": {"0": {"create_canvas": {"w": 64, "h": 64, "format": "bgra_32", "color": "transparent"}},
                                       "1": {"fill_rect": {"x1": 0, "y1": 0, "x2": 10, "y2": 10, "color": {"srgb": {"hex": "EECCFFFF"}}}},
                                       "2": {"constrain": {"mode": "within", "w": 32}}, "3": {"command_string": {"kind": "ir4", "value": "width=20&mode=max"}}},
                             "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 1, "to": 2, "kind": "input"}, {"from": 2, "to": 3, "kind": "input"}]}}},
]

INVALID_BODIES = [b"{bad", b"", b'{"framewise": ', b'{"a": 1} trailing', b'{"framewise":{"steps":[{"decode":{"io_id":"x"}}]}}', b"[" * 100 + b"]" * 100]
GRAMMAR_NUMBERS = [b"inf", b"Infinity", b"nan", b"0x10", b"+1", b"1e999", b"01", b"1.", b".5", b"-"]
