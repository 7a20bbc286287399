"""ctypes signatures of the native C API, declared once: every `extern "C"` `tv_*` function
of ``libtvcore.so`` (csrc/core) and ``libtvgpu.so`` (csrc/gpu) as name -> (restype, [argtypes]).
:mod:`thinvids_amd._native` applies ``CORE`` / ``GPU`` when it loads a library, so ctypes refuses
a call with the wrong number or kind of arguments before any native code runs;
tests/test_abi.py checks both tables against the C sources, which are the authority.

Device pointers, streams and opaque handles are ``c_void_p`` (callers pass ``tensor.data_ptr()``
as a plain int); host arrays keep a typed ``POINTER``; ``void`` returns are ``None``.
"""
import ctypes as C

i, l, ll, sz, ull, f32 = C.c_int, C.c_long, C.c_longlong, C.c_size_t, C.c_ulonglong, C.c_float
i32, i64, u32, vp, cstr = C.c_int32, C.c_int64, C.c_uint32, C.c_void_p, C.c_char_p
u8p, i8p, i16p, i32p, u32p = (C.POINTER(t) for t in (C.c_uint8, C.c_int8, C.c_int16, C.c_int32, C.c_uint32))
i64p, u64p, lp, llp, ullp, szp = (C.POINTER(t) for t in (C.c_int64, C.c_uint64, l, ll, ull, sz))
f64p, vpp = C.POINTER(C.c_double), C.POINTER(vp)


class SideTrack(C.Structure):
    """Mirror of `SideTrack` (csrc/include/tv/container.h); core_lib() checks its size."""
    _fields_ = [("kind", i32), ("codec", i32), ("timescale", i32), ("channels", i32), ("sample_rate", i32),
                ("bits", i32), ("is_default", i32), ("reserved", i32), ("lang", C.c_char * 4), ("mkv_codec_id", cstr),
                ("priv", vp), ("priv_size", C.c_uint64), ("path", cstr), ("data", vp), ("nsamples", i64),
                ("offsets", vp), ("sizes", vp), ("pts", vp), ("durs", vp)]


CORE = {
    # capi.cpp: errors, byte vectors, synthetic source
    "tv_core_build_hash": (cstr, []),
    "tv_last_error": (cstr, []),
    "tv_core_version": (i, []),
    "tv_bytes_new": (vp, []),
    "tv_bytes_free": (None, [vp]),
    "tv_bytes_size": (sz, [vp]),
    "tv_bytes_data": (vp, [vp]),
    "tv_bytes_clear": (None, [vp]),
    "tv_synth_frame": (None, [u32, i, i, i, u8p, u8p, u8p]),
    "tv_synth_frame_tiled": (None, [u32, i, i, i, i, i, u8p, u8p, u8p]),
    "tv_satd8x8": (i, [i32p, i]),
    "tv_sao_picture_cpu": (i, [i, i, i] + [u8p] * 6 + [u32p] + [u8p] * 3),
    # HEVC golden encoder
    "tv_cpu_encoder_new": (vp, [i] * 6),
    "tv_cpu_encoder_new_b": (vp, [i] * 7),
    "tv_cpu_encoder_new_crf": (vp, [i] * 7),
    "tv_cpu_encoder_free": (None, [vp]),
    "tv_cpu_encoder_begin_gop": (i, [vp, i, i32p]),
    "tv_gop_plan": (i, [i, i] + [i32p] * 6),
    "tv_cpu_encoder_encode": (i, [vp, u8p, u8p, u8p, i, i, i, i, vp]),
    "tv_cpu_encoder_encode_qp": (i, [vp, u8p, u8p, u8p, i, i, i, i, i, vp]),
    "tv_cpu_encoder_recon": (None, [vp, u8p, u8p, u8p]),
    "tv_cpu_encoder_decisions": (None, [vp, u8p, u8p, u8p, i16p, u8p]),
    "tv_cpu_encoder_levels": (None, [vp, i16p, i16p, i16p]),
    "tv_reconstruct_frame": (i, [i] * 4 + [u8p] * 9 + [i16p, u8p, i16p, i16p, i16p, u8p, u8p, u8p]),
    "tv_write_frame": (i, [i] * 7 + [u8p, u8p, u8p, i16p, u8p, i16p, i16p, i16p, vp]),
    "tv_mv_rate": (None, [i32p, i32p, i, i32p, i32p]),
    "tv_av1_mv_comp_bits": (None, [i32p, i, i32p]),
    "tv_tb_frag_expand": (i, [i, i32p]),
    "tv_quant_levels": (None, [i32p, i, i, i, i32p, i32p]),
    "tv_sdh_deltas": (None, [i32p, i, i, i, i, i32p, i32p]),
    "tv_rdq_tb": (i, [i32p, i, i, i, i, i16p, llp]),
    "tv_hevc_spec_table": (i, [cstr, i32p, i]),
    # HEVC decoder
    "tv_decoder_new": (vp, []),
    "tv_decoder_free": (None, [vp]),
    "tv_decoder_decode": (i, [vp, u8p, sz]),
    "tv_decoder_decode_range": (i, [vp, u8p, sz, i, i]),
    "tv_decoder_info": (None, [vp] + [i32p] * 5),
    "tv_decoder_frame": (i, [vp, i, i, u8p, u8p, u8p]),
    "tv_hevc_scale_mv": (None, [i, i, i, i, i32p]),
    "tv_hevc_display_offsets": (i, [u8p, sz, i32p, i]),
    "tv_hevc_probe": (i, [u8p, sz] + [i32p] * 4),
    # containers and file I/O
    "tv_mux_mp4": (i, [u8p, sz, i, i, i, i, vp]),
    "tv_mux_mp4_file": (i, [vpp, szp, i, i, i, i, i, cstr, ullp]),
    "tv_mux_file": (i, [vpp, szp, i, i, i, i, i, C.POINTER(SideTrack), i, i, cstr, ullp]),
    "tv_side_track_size": (sz, []),
    "tv_demux_mp4": (i, [u8p, sz] + [i32p] * 5 + [vp]),
    "tv_mp4s_open": (vp, [cstr, i, i, i, i, ull]),
    "tv_mp4s_append": (i, [vp, u8p, sz]),
    "tv_mp4s_close": (i, [vp, ullp]),
    "tv_mp4s_abort": (None, [vp]),
    "tv_mp4s_last_error": (cstr, []),
    "tv_io_last_error": (cstr, []),
    "tv_pread_parallel": (ll, [cstr, ll, ll, vp, i]),
    "tv_readahead": (i, [cstr, ll, ll]),
    # AV1 codec golden model
    "tv_av1c_last_error": (cstr, []),
    "tv_av1c_qlookup": (i, [i, i]),
    "tv_av1c_model_constants": (i, [i64p]),
    "tv_av1c_model_q": (None, [i, i64p]),
    "tv_av1c_golden_encode": (i, [i, i, i, u8p, i, i32p, i, vp, i64p, u8p, u32p, u32p, i16p, i16p, i16p, i32p, i8p,
                                  i32p, u8p]),
    "tv_av1c_ib_accept": (i, [u8p, i, i, u8p]),
    "tv_av1c_cfl_decide": (i, [u8p, u8p, u8p, i, i, i, i, i32p]),
    "tv_av1c_dir_predict": (i, [i, u8p, i, i, i, i, u8p]),
    "tv_av1c_dir_tables": (None, [i32p] * 5),
    "tv_av1c_dir_cands": (None, [i32p]),
    "tv_av1c_dir_decide": (i, [i, u8p, u8p, u8p, u8p, i, i, i, i, i, i, i, i32p, i32p]),
    "tv_av1c_tx_split_decide": (i, [u8p, u8p, i, i, i16p, u8p, i16p, u8p, i64p]),
    "tv_av1c_decode": (i, [u8p, sz, i, u8p, i32p, i32p]),
    "tv_av1c_decode_modes": (i, [u8p, sz, i, u32p, u32p]),
    "tv_av1c_probe": (i, [u8p, sz, i32p, i32p]),
    "tv_av1c_state_new": (vp, []),
    "tv_av1c_state_free": (None, [vp]),
    "tv_av1c_write_tu": (i, [vp, i, i, i32p, u32p, u32p, i16p, i16p, i16p, i8p, i32p, i, i, vp]),
    # AV1 in-loop filter and transform golden models
    "tv_av1_last_error": (cstr, []),
    "tv_av1_cdef_find_dirs": (None, [u8p, i, i, u8p, i32p]),
    "tv_av1_cdef_search": (None, [u8p, u8p, i, i, i, u8p, i32p, i, i, u64p]),
    "tv_av1_cdef_apply": (None, [u8p, i, i, i, u8p, i32p, i, i, i8p, u8p]),
    "tv_av1_wiener_apply": (None, [u8p, i, i, i32p, u8p]),
    "tv_av1_wiener_stats": (None, [u8p, u8p, i, i, i, i32p, i64p]),
    "tv_av1_sgr_apply": (None, [u8p, i, i, i32p, u8p]),
    "tv_av1_sgr_stats": (None, [u8p, u8p, i, i, i, i64p]),
    "tv_av1_sgr_filter_planes": (None, [u8p, i, i, i, i32p, i32p]),
    "tv_av1_deblock": (i, [u8p, i, i, i, u32p, i, u8p]),
    "tv_av1_rc_roundtrip": (i, [i32p, i32p, i32p, i, i, i, vp, i32p]),
    "tv_av1_txfm_ref": (i, [i16p, i16p, i, i, i, i, i]),
    "tv_av1_txfm_basis": (i, [i, i, i32p]),
    # MPEG-2
    "tv_mpeg2_last_error": (cstr, []),
    "tv_mpeg2_encode": (i, [i32p, i, i, u8p, vp, i64p, i32p, u8p]),
    "tv_mpeg2_probe": (i, [u8p, sz, i32p]),
    "tv_mpeg2_raps": (i, [u8p, sz, i64p, i64p, i32p, i32p, i]),
    "tv_mpeg2_decode": (i, [u8p, sz, i64, i64, i32, i32, i32, u8p, i32p, i64p]),
    "tv_mpeg2_table": (i, [i, i32p, i32p, i32p, i]),
    "tv_mpeg2_stat_name": (cstr, [i]),
    "tv_mpeg2_num_stats": (i, []),
}

GPU = {
    # engine.hip: the HEVC engine (handle first; host arrays typed)
    "tv_gpu_build_hash": (cstr, []),
    "tv_gpu_last_error": (cstr, []),
    "tv_gpu_device_count": (i, []),
    "tv_engine_new_b": (vp, [i] * 7 + [u32, i, i, i, i, i]),
    "tv_engine_free": (None, [vp]),
    "tv_engine_encode_synth": (i, [vp, i32p, i, i, vp]),
    "tv_engine_encode_host": (i, [vp, u8p, i, i, vp]),
    "tv_engine_encode_device": (i, [vp, vp, i, i, vp]),
    "tv_engine_segment_size": (sz, [vp, i]),
    "tv_engine_segment_copy": (None, [vp, i, u8p]),
    "tv_engine_sse": (None, [vp, i, f64p]),
    "tv_engine_timing": (None, [vp] + [f64p] * 4),
    "tv_engine_entropy_stats": (None, [vp, i32p, llp, i32p]),
    "tv_engine_entropy_host_pictures": (ll, [vp]),
    "tv_engine_entropy_lane_pictures": (ll, [vp, i]),
    "tv_engine_estimate": (i, [i] * 6 + [ullp, ullp]),
    "tv_engine_footprint": (None, [vp, ullp, ullp]),
    "tv_engine_last_recon": (i, [vp, i, u8p, u8p, u8p]),
    # ingest.hip, k_stage.hip
    "tv_ingest_last_error": (cstr, []),
    "tv_ingest_h2d": (i, [cstr, ll, ll, vp, vp, ll, i, vp, f64p]),
    "tv_stage_last_error": (cstr, []),
    "tv_thumbs8_batch": (i, [vp, i, i, i, i, l, i, vp, vp]),
    "tv_pad_batch": (i, [vp, i, i, i, l, vp, i, i, i, l, i, vp]),
    "tv_synth_batch": (i, [vp, i, i, i, i32p, u32, vp]),
    "tv_sao_batch": (i, [vp, vp, vp, vp, vp, i, i, i, i8p, vp]),
    # k_ops.hip: every pointer is a device pointer or the stream, but the bwdif plane tables
    "tv_ops_last_error": (cstr, []),
    "tv_resize_plane": (i, [vp, i, i, i, vp, i, i, i, vp, vp, i, vp, vp, i, vp, vp]),
    "tv_resize_batch": (i, [vp, i, i, i, l, vp, i, i, i, l, i, i, i, vp, vp, i, vp, vp, i, vp, i, i, i, vp]),
    "tv_rgb_to_i420": (i, [vp, i, i, i, vp, vp, vp, i, vp]),
    "tv_p010_to_i420": (i, [vp, vp, i, i, vp, vp, vp, vp]),
    "tv_tonemap_pq": (i, [vp, vp, i, i, vp, vp, vp, f32, f32, vp]),
    "tv_tonemap_pq_batch": (i, [vp, vp, i, i, i, vp, f32, f32, vp]),
    "tv_synth_p010": (i, [vp, vp, i, i, i, i, u32, vp]),
    "tv_overlay_mask": (i, [vp, i, i, i, vp, i, i, i, i, vp]),
    "tv_bwdif_segment": (i, [vp, vp, l, i, i, lp, i32p, i32p, i, vp]),
    "tv_bwdif_plane": (i, [vp, vp, vp, vp, i, i, i, vp]),
    "tv_ssim_plane": (i, [vp, vp, i, i, i, i, vp, vp]),
    # k_av1.hip, k_av1_txfm.hip: AV1 in-loop filters and transforms (device pointers and the stream)
    "tv_av1_gpu_last_error": (cstr, []),
    "tv_gpu_cdef_dirs": (i, [vp, i, i, i, vp, vp, vp]),
    "tv_gpu_cdef_search": (i, [vp, vp, i, i, i, i, vp, vp, i, i, i, vp, vp, ull, i]),
    "tv_gpu_cdef_apply": (i, [vp, i, i, i, i, vp, vp, i, i, i, vp, vp, vp]),
    "tv_gpu_sgr_select": (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, vp]),
    "tv_gpu_wiener_apply": (i, [vp, i, i, i, vp, vp, vp]),
    "tv_gpu_wiener_stats": (i, [vp, vp, i, i, i, i, vp, vp, vp]),
    "tv_gpu_sgr_stats": (i, [vp, vp, i, i, i, i, vp, vp]),
    "tv_gpu_sgr_apply": (i, [vp, i, i, i, vp, vp, vp]),
    "tv_gpu_av1_deblock_step": (i, [vp, vp, i, i, i, i, vp, i, i, vp]),
    "tv_av1_txfm_last_error": (cstr, []),
    "tv_gpu_av1_txfm": (i, [vp, vp, i, i, i, vp, vp, vp]),
    # k_av1_enc.hip: the AV1 engine (device pointers, stream last)
    "tv_av1e_last_error": (cstr, []),
    "tv_av1e_inter": (i, [vp] * 18 + [i, i, i, vp, vp]),
    "tv_av1e_inter_tools": (i, [vp] * 18 + [i, i, i, vp, i, vp]),
    "tv_av1e_iblocks": (i, [vp] * 16 + [i, i, i, vp, i, vp]),
    "tv_av1e_intra": (i, [vp] * 11 + [i, i, i, vp, i, vp]),
    "tv_av1e_cdef_skip": (i, [vp, vp, i, i, i, vp]),
    "tv_av1e_merge": (i, [vp, vp, i, i, i, vp]),
    "tv_av1e_tb_len": (i, [vp, vp, l, i, i, i, i, vp, vp]),
    "tv_av1e_tb_pack": (i, [vp, vp, vp, vp, l, i, i, i, i, vp, vp]),
    "tv_av1e_lfinfo": (i, [vp, i, i, i, vp, vp, vp, vp, vp]),
    "tv_av1e_unit_sse": (i, [vp, vp, i, i, i, i, i, vp, vp]),
    "tv_av1e_cdef_choose": (i, [vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]),
}
