"""Loader for libsoundkit_amd.so (the C ABI of include/soundkit_amd.h).

The HIP library is the product; there is no Python or CPU compute fallback.  If the
shared object is missing or cannot be loaded this module raises ImportError loudly.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOUNDKIT_AMD_LIB") or os.path.join(_HERE, "libsoundkit_amd.so")  # override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "soundkit_amd.h")

SK_OK = 0
AAC_UNIT_SIDE_BYTES = 1600  # SK_AAC_UNIT_SIDE_BYTES
ERR_NAMES = {0: "SK_OK", -1: "SK_ERR_INVALID_ARG", -2: "SK_ERR_NO_DEVICE", -3: "SK_ERR_HIP", -4: "SK_ERR_OOM",
             -5: "SK_ERR_BAD_STREAM", -6: "SK_ERR_UNSUPPORTED", -7: "SK_ERR_CAPACITY", -8: "SK_ERR_TIMEOUT", -9: "SK_ERR_INTERNAL",
             -101: "UnexpectedEof", -102: "InvalidAudioObjectType", -103: "UnsupportedAudioObjectType",
             -104: "UnsupportedSamplingFrequencyIndex", -105: "UnsupportedChannelConfig", -106: "UnsupportedFeature",
             -107: "InvalidConfig", -108: "InvalidBitstream",
             -301: "Mp3NeedMore", -302: "Mp3NoSync", -303: "Mp3Unsupported", -304: "Mp3Invalid",
             -401: "PcmStreamRejected",
             -501: "FlacNeedMore", -502: "FlacNoSync", -503: "FlacReserved", -504: "FlacBadCrc", -505: "FlacNeedStreamInfo",
             -506: "FlacInvalid", -507: "FlacStreamRejected",
             -601: "AlacInvalid", -602: "AlacStreamRejected", -603: "AlacUnsupportedElement",
             -701: "TelephonyStreamRejected",
             -801: "VorbisNotAudio", -802: "VorbisBadMode", -803: "VorbisPacketShort", -804: "VorbisStreamRejected",
             -901: "Mp4StreamRejected",
             -1001: "WebmStreamRejected",
             -1101: "TsStreamRejected",
             -1201: "WavBadBlock",
             -1301: "CafStreamRejected",
             -1401: "AviStreamRejected",
             -1501: "PsStreamRejected",
             -201: "InputBufferFull", -202: "PipelineClosed", -203: "InputChunkTooLarge"}


class FrameDesc(C.Structure):
    """sk_aac_frame_desc"""
    _fields_ = [("stream", C.c_uint32), ("channels", C.c_uint8), ("window_sequence", C.c_uint8 * 2),
                ("window_shape", C.c_uint8 * 2), ("reserved", C.c_uint8 * 3)]


class Mp3GranuleDesc(C.Structure):
    """sk_mp3_granule_desc"""
    _fields_ = [("stream", C.c_uint32), ("channels", C.c_uint8), ("block_type", C.c_uint8 * 2), ("mixed_block_flag", C.c_uint8 * 2),
                ("reserved", C.c_uint8 * 3)]


class Mp3FrameInfo(C.Structure):
    """sk_mp3_frame_info"""
    _fields_ = [("offset", C.c_uint32), ("frame_bytes", C.c_uint32), ("sample_rate", C.c_uint32), ("bitrate_kbps", C.c_uint16),
                ("samples_per_channel", C.c_uint16)] + [(n, C.c_uint8) for n in ("version", "channels", "mode", "mode_ext", "has_crc",
                                                                                  "padding", "granules", "side_info_bytes")]


class Mp3GranuleSide(C.Structure):
    """sk_mp3_granule_side"""
    _fields_ = [("part2_3_length", C.c_uint16), ("big_values", C.c_uint16), ("scalefac_compress", C.c_uint16), ("global_gain", C.c_uint8),
                ("window_switching", C.c_uint8), ("block_type", C.c_uint8), ("mixed_block_flag", C.c_uint8), ("table_select", C.c_uint8 * 3),
                ("subblock_gain", C.c_uint8 * 3), ("region0_count", C.c_uint8), ("region1_count", C.c_uint8), ("preflag", C.c_uint8),
                ("scalefac_scale", C.c_uint8), ("count1table_select", C.c_uint8), ("reserved", C.c_uint8)]


class Mp3SideInfo(C.Structure):
    """sk_mp3_side_info"""
    _fields_ = [("main_data_begin", C.c_uint16), ("granules", C.c_uint8), ("channels", C.c_uint8), ("scfsi", (C.c_uint8 * 4) * 2),
                ("gr", (Mp3GranuleSide * 2) * 2)]


class Mp3RequantChannel(C.Structure):
    """sk_mp3_requant_channel"""
    _fields_ = [("global_gain", C.c_uint8), ("scalefac_scale", C.c_uint8), ("preflag", C.c_uint8), ("block_type", C.c_uint8),
                ("mixed_block_flag", C.c_uint8), ("subblock_gain", C.c_uint8 * 3), ("scalefac_l", C.c_uint8 * 22),
                ("scalefac_s", (C.c_uint8 * 3) * 13), ("reserved", C.c_uint8)]


class Mp3RequantGranule(C.Structure):
    """sk_mp3_requant_granule"""
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("ms_stereo", C.c_uint8), ("intensity_stereo", C.c_uint8),
                ("lsf", C.c_uint8), ("ch", Mp3RequantChannel * 2)]


class Mp3CodeTable(C.Structure):
    """sk_mp3_code_table"""
    _fields_ = [("xlen", C.c_uint8), ("linbits", C.c_uint8), ("hlen", C.POINTER(C.c_uint8)), ("hcod", C.POINTER(C.c_uint32))]


class Mp3Tables(C.Structure):
    """sk_mp3_tables"""
    _fields_ = [("big_values", Mp3CodeTable * 32), ("count1_hlen", (C.c_uint8 * 16) * 2), ("count1_hcod", (C.c_uint8 * 16) * 2),
                ("slen", (C.c_uint8 * 2) * 16), ("lsf_partitions", ((C.c_uint8 * 4) * 3) * 6), ("long_offsets", (C.c_uint16 * 23) * 9),
                ("short_offsets", (C.c_uint16 * 14) * 9), ("rates_present", C.c_uint8 * 9), ("pretab", C.c_uint8 * 22),
                ("window", C.c_float * 512)]


class Mp3GranuleData(C.Structure):
    """sk_mp3_granule_data"""
    _fields_ = [("is_", C.c_int16 * 576), ("scalefac_l", C.c_uint8 * 22), ("scalefac_s", (C.c_uint8 * 3) * 13), ("preflag", C.c_uint8),
                ("intensity_scale", C.c_uint8), ("part2_bits", C.c_uint16), ("nonzero_lines", C.c_uint16), ("part3_bits", C.c_uint16), ("status", C.c_int32)]


class Mp3FrameItem(C.Structure):
    """sk_mp3_frame_item"""
    _fields_ = [("header", Mp3FrameInfo), ("side", Mp3SideInfo), ("byte_offset", C.c_uint32), ("byte_len", C.c_uint32)]


class MpaFrameInfo(C.Structure):
    """sk_mpa_frame_info"""
    _fields_ = [("offset", C.c_uint32), ("frame_bytes", C.c_uint32), ("sample_rate", C.c_uint32), ("bitrate_kbps", C.c_uint16),
                ("samples_per_channel", C.c_uint16)] + [(n, C.c_uint8) for n in ("version", "layer", "channels", "mode", "mode_ext", "has_crc",
                                                                                  "padding", "reserved")]


class MpaFrameRecord(C.Structure):
    """sk_mpa_frame_record"""
    _fields_ = [("byte_offset", C.c_uint32), ("byte_len", C.c_uint32), ("sample_rate", C.c_uint32), ("sample_bit", C.c_uint32),
                ("granule_bits", C.c_uint16)] + [(n, C.c_uint8) for n in ("layer", "channels", "sblimit", "bound", "granules", "reserved")] + [
                    ("cls", (C.c_uint8 * 32) * 2), ("scf", ((C.c_uint8 * 3) * 32) * 2)]


class TickMp3Frames(C.Structure):
    """sk_tick_mp3_frames"""
    _fields_ = [("frames", C.c_void_p), ("n_frames", C.c_uint32), ("main_bytes", C.c_void_p), ("main_len", C.c_size_t)]


class TickMpaFrames(C.Structure):
    """sk_tick_mpa_frames"""
    _fields_ = [("records", C.c_void_p), ("n_frames", C.c_uint32), ("frame_bytes", C.c_void_p), ("bytes_len", C.c_size_t)]


class TickStream(C.Structure):
    """sk_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_frames", C.c_uint32), ("out_bits", C.c_uint8), ("out_channels", C.c_uint8),
                ("resample", C.c_uint8), ("flush", C.c_uint8), ("codec", C.c_uint8), ("reserved", C.c_uint8 * 3)]


SK_TICK_AAC, SK_TICK_MP3, SK_TICK_MPA = 0, 1, 2  # sk_tick_stream.codec


class TickInput(C.Structure):
    """sk_tick_input"""
    _fields_ = [("descs", C.c_void_p), ("coeffs", C.c_void_p), ("units", C.c_void_p), ("au_bytes", C.c_void_p), ("au_bytes_len", C.c_size_t),
                ("q_sides", C.c_void_p), ("q_quant", C.c_void_p), ("n_aac_units", C.c_uint32), ("n_mp3_granules", C.c_uint32),
                ("mp3_granules", C.c_void_p), ("mp3_descs", C.c_void_p), ("mp3_is", C.c_void_p)]


class TickOutput(C.Structure):
    """sk_tick_output"""
    _fields_ = [("stream_index", C.c_uint32), ("frames", C.c_uint32), ("byte_offset", C.c_uint64), ("bytes", C.c_uint32),
                ("status", C.c_int32), ("channels", C.c_uint8), ("bits", C.c_uint8), ("reserved", C.c_uint16)]


class PcmTickStream(C.Structure):
    """sk_pcm_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("format", C.c_uint8), ("channels", C.c_uint8), ("out_bits", C.c_uint8),
                ("out_channels", C.c_uint8), ("resample", C.c_uint8), ("flush", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class PcmUnit(C.Structure):
    """sk_pcm_unit"""
    _fields_ = [("byte_offset", C.c_uint64), ("byte_len", C.c_uint32), ("reserved", C.c_uint32)]


class AiffImaState(C.Structure):
    """sk_aiff_ima_state"""
    _fields_ = [("predictor", C.c_int16), ("step_index", C.c_uint8), ("reserved", C.c_uint8)]


class AiffTickStream(C.Structure):
    """sk_aiff_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("encoding", C.c_uint8), ("channels", C.c_uint8), ("out_bits", C.c_uint8),
                ("out_channels", C.c_uint8), ("resample", C.c_uint8), ("flush", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("ima_state", AiffImaState * 2)]


class AiffInfo(C.Structure):
    """sk_aiff_info"""
    _fields_ = [("sample_rate", C.c_uint32), ("buffered_bytes", C.c_uint32), ("channels", C.c_uint8), ("encoding", C.c_uint8),
                ("bits", C.c_uint8), ("is_float", C.c_uint8)]


class WavCodedInfo(C.Structure):
    """sk_wav_coded_info"""
    _fields_ = [(n, C.c_uint32) for n in ("tag", "sample_rate", "channels", "bits", "is_float", "block_align", "frames_per_block", "n_coef")] + [
        ("coef", (C.c_int16 * 2) * 32), ("fact_frames", C.c_uint32), ("reserved", C.c_uint32), ("total_frames", C.c_uint64)]


class WavAdpcmTickStream(C.Structure):
    """sk_wav_adpcm_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("tag", C.c_uint16), ("channels", C.c_uint8), ("out_bits", C.c_uint8),
                ("out_channels", C.c_uint8), ("resample", C.c_uint8), ("flush", C.c_uint8), ("n_coef", C.c_uint8), ("block_align", C.c_uint32),
                ("frames_per_block", C.c_uint32), ("frames_left", C.c_uint64), ("coef", (C.c_int16 * 2) * 32)]


class FlacStreamInfo(C.Structure):
    """sk_flac_streaminfo"""
    _fields_ = [(n, C.c_uint32) for n in ("min_blocksize", "max_blocksize", "min_framesize", "max_framesize", "sample_rate")] + [
        ("channels", C.c_uint8), ("bits_per_sample", C.c_uint8), ("reserved", C.c_uint16), ("total_samples", C.c_uint64), ("md5", C.c_uint8 * 16)]


class FlacFrameInfo(C.Structure):
    """sk_flac_frame_info"""
    _fields_ = [("number", C.c_uint64), ("offset", C.c_uint32), ("frame_bytes", C.c_uint32), ("sample_rate", C.c_uint32),
                ("block_size", C.c_uint32)] + [(n, C.c_uint8) for n in ("header_bytes", "channels", "assignment", "bits_per_sample",
                                                                         "variable_blocksize")] + [("reserved", C.c_uint8 * 3)]


class FlacInfo(C.Structure):
    """sk_flac_info"""
    _fields_ = [("streaminfo", FlacStreamInfo), ("frames", C.c_uint64), ("buffered_bytes", C.c_uint32), ("have_streaminfo", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class AlacConfig(C.Structure):
    """sk_alac_config"""
    _fields_ = [(n, C.c_uint32) for n in ("frame_length", "sample_rate", "max_frame_bytes", "avg_bit_rate")] + [("max_run", C.c_uint16)] + [
        (n, C.c_uint8) for n in ("compatible_version", "bit_depth", "pb", "mb", "kb", "channels")]


class CafAlacInfo(C.Structure):
    """sk_caf_alac_info"""
    _fields_ = [("config", AlacConfig), ("valid_frames", C.c_uint64), ("priming_frames", C.c_uint32), ("remainder_frames", C.c_uint32),
                ("frames_per_packet", C.c_uint32), ("n_packets", C.c_uint32)]


class Mp4TrackInfo(C.Structure):
    """sk_mp4_track_info"""
    _fields_ = [(n, C.c_uint32) for n in ("codec", "sample_rate", "channels", "bits_per_sample", "track_id", "timescale", "sample_count",
                                          "fragmented", "has_edit", "private_len")] + [
        (n, C.c_uint64) for n in ("edit_presentation_start", "edit_media_start", "edit_duration")]


class Mp4PcmInfo(C.Structure):
    """sk_mp4_pcm_info"""
    _fields_ = [("codec_id", C.c_char * 4)] + [(n, C.c_uint32) for n in ("big_endian", "is_float", "bits_per_sample", "bytes_per_frame", "frames_per_packet")]


class CafInfo(C.Structure):
    """sk_caf_info"""
    _fields_ = [("codec", C.c_uint32), ("format_id", C.c_char * 4)] + [(n, C.c_uint32) for n in (
        "sample_rate", "channels", "bits_per_sample", "format_flags", "big_endian", "is_float", "bytes_per_frame", "frames_per_packet",
        "priming_frames", "remainder_frames", "n_packets", "cookie_len")] + [("valid_frames", C.c_uint64)]


class WebmTrackInfo(C.Structure):
    """sk_webm_track_info"""
    _fields_ = [(n, C.c_uint64) for n in ("track_number", "codec_delay_ns", "seek_pre_roll_ns", "default_duration_ns", "timecode_scale_ns")] + [
        ("track_timestamp_scale", C.c_double)] + [(n, C.c_uint32) for n in ("codec", "sample_rate", "channels", "private_len", "prefix_len", "reserved")]


class WebmPacketInfo(C.Structure):
    """sk_webm_packet_info"""
    _fields_ = [("track_number", C.c_uint64), ("timestamp_ns", C.c_int64), ("duration_ns", C.c_uint64), ("discard_padding_ns", C.c_int64),
                ("codec", C.c_uint32), ("has_duration", C.c_uint8), ("has_discard_padding", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class TsTrackInfo(C.Structure):
    """sk_ts_track_info"""
    _fields_ = [(n, C.c_uint32) for n in ("codec", "packet_format", "stream_type", "pid", "program_number", "packet_stride", "packet_prefix", "sample_rate",
                                          "channels", "bits_per_sample", "bytes_per_frame", "frames_per_packet")] + [
        ("has_rate", C.c_uint8), ("has_channels", C.c_uint8), ("lpcm_header", C.c_uint8 * 4), ("reserved", C.c_uint8 * 2)]


class TsPacketInfo(C.Structure):
    """sk_ts_packet_info"""
    _fields_ = [("pts", C.c_uint64), ("dts", C.c_uint64), ("duration", C.c_uint32), ("has_pts", C.c_uint8), ("has_dts", C.c_uint8), ("has_duration", C.c_uint8),
                ("continuity_counter", C.c_uint8), ("discontinuity", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class AviTrackInfo(C.Structure):
    """sk_avi_track_info"""
    _fields_ = [("stream_index", C.c_uint32), ("sample_rate", C.c_uint32), ("format_tag", C.c_uint16), ("channels", C.c_uint8), ("bits", C.c_uint8)]


class PsTrackInfo(C.Structure):
    """sk_ps_track_info"""
    _fields_ = [("sample_rate", C.c_uint32), ("block_bytes", C.c_uint32), ("kind", C.c_uint8), ("stream_id", C.c_uint8), ("substream_id", C.c_uint8),
                ("channels", C.c_uint8), ("bits", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class AlacTickStream(C.Structure):
    """sk_alac_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("frame_length", C.c_uint32)] + [
        (n, C.c_uint8) for n in ("channels", "bit_depth", "pb", "mb", "kb", "out_bits", "out_channels", "resample", "flush")] + [("reserved", C.c_uint8 * 3)]


class AlacTickPacket(C.Structure):
    """sk_alac_tick_packet"""
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32), ("frames", C.c_uint32), ("reserved", C.c_uint32)]


class AlacPacket(C.Structure):
    """sk_alac_packet"""
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32)]


class G726State(C.Structure):
    """sk_g726_state"""
    _fields_ = [(n, C.c_int32) for n in ("yl", "yu", "dms", "dml", "ap")] + [("a", C.c_int32 * 2), ("b", C.c_int32 * 6), ("pk", C.c_int32 * 2),
                                                                              ("dq", C.c_int32 * 6), ("sr", C.c_int32 * 2), ("td", C.c_int32)]


class G722Band(C.Structure):
    """sk_g722_band"""
    _fields_ = [("s", C.c_int32), ("sz", C.c_int32), ("r", C.c_int32 * 2), ("p", C.c_int32 * 2), ("a", C.c_int32 * 2), ("b", C.c_int32 * 6),
                ("d", C.c_int32 * 6), ("nb", C.c_int32), ("det", C.c_int32)]


class G722State(C.Structure):
    """sk_g722_state"""
    _fields_ = [("band", G722Band * 2), ("x", C.c_int32 * 22)]


class G72xStream(C.Structure):
    """sk_g72x_stream"""
    _fields_ = [("codec", C.c_uint8), ("g726_packing", C.c_uint8), ("reserved", C.c_uint8 * 2), ("g726_rate", C.c_uint32), ("n_units", C.c_uint32),
                ("state", C.c_uint32)]


class G72xUnit(C.Structure):
    """sk_g72x_unit"""
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32), ("out_len", C.c_uint32), ("reserved", C.c_uint32), ("out_offset", C.c_uint64)]


class G72xTickStream(C.Structure):
    """sk_g72x_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("g726_rate", C.c_uint32), ("state", C.c_uint32)] + [
        (n, C.c_uint8) for n in ("codec", "g726_packing", "channels", "out_bits", "out_channels", "resample", "flush", "reserved")]


class GsmState(C.Structure):
    """sk_gsm_state"""
    _fields_ = [("dp", C.c_int32 * 120), ("v", C.c_int32 * 8), ("msr", C.c_int32), ("nrp", C.c_int32), ("larpp", C.c_int32 * 8)]


class GsmStream(C.Structure):
    """sk_gsm_stream"""
    _fields_ = [("variant", C.c_uint32), ("n_units", C.c_uint32), ("state", C.c_uint32)]


class GsmTickStream(C.Structure):
    """sk_gsm_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("state", C.c_uint32)] + [
        (n, C.c_uint8) for n in ("variant", "channels", "out_bits", "out_channels", "resample", "flush")] + [("reserved", C.c_uint8 * 2)]


class FlacTickStream(C.Structure):
    """sk_flac_tick_stream"""
    _fields_ = [("stream", C.c_uint32), ("n_units", C.c_uint32), ("channels", C.c_uint8), ("bits_per_sample", C.c_uint8), ("out_bits", C.c_uint8),
                ("out_channels", C.c_uint8), ("resample", C.c_uint8), ("flush", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class OggPacketInfo(C.Structure):
    """sk_ogg_packet_info"""
    _fields_ = [("granule_position", C.c_uint64), ("size", C.c_uint32), ("serial", C.c_uint32)] + [
        (n, C.c_uint8) for n in ("first_in_stream", "last_in_page", "last_in_stream", "has_granule")] + [("reserved", C.c_uint8 * 4)]


class VorbisIdent(C.Structure):
    """sk_vorbis_ident"""
    _fields_ = [(n, C.c_uint32) for n in ("sample_rate", "bitrate_maximum", "bitrate_nominal", "bitrate_minimum")] + [
        ("blocksize_0", C.c_uint16), ("blocksize_1", C.c_uint16), ("channels", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class VorbisSetupInfo(C.Structure):
    """sk_vorbis_setup_info"""
    _fields_ = [(n, C.c_uint32) for n in ("books", "floors", "residues", "mappings", "modes", "blob_bytes")] + [
        ("blocksize_0", C.c_uint16), ("blocksize_1", C.c_uint16), ("channels", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class VorbisStream(C.Structure):
    """sk_vorbis_stream"""
    _fields_ = [("setup", C.c_void_p), ("overlap", C.c_void_p), ("n_packets", C.c_uint32), ("prev_blocksize", C.c_uint32)]


class VorbisTickStream(C.Structure):
    """sk_vorbis_tick_stream"""
    _fields_ = [("setup", C.c_void_p), ("overlap", C.c_void_p), ("stream", C.c_uint32), ("n_units", C.c_uint32), ("prev_blocksize", C.c_uint32)] + [
        (n, C.c_uint8) for n in ("out_bits", "out_channels", "resample", "flush", "channels")] + [("reserved", C.c_uint8 * 3)]


class VorbisTickPacket(C.Structure):
    """sk_vorbis_tick_packet"""
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32), ("keep_frames", C.c_uint32), ("skip_frames", C.c_uint32)]


class VorbisPacket(C.Structure):
    """sk_vorbis_packet"""
    _fields_ = [("offset", C.c_uint32), ("size", C.c_uint32)]


class VorbisPacketInfo(C.Structure):
    """sk_vorbis_packet_info"""
    _fields_ = [("status", C.c_int32), ("mode", C.c_uint8), ("blockflag", C.c_uint8), ("prev_flag", C.c_uint8), ("next_flag", C.c_uint8),
                ("blocksize", C.c_uint32), ("used", C.c_uint8 * 8), ("final_y", (C.c_int16 * 65) * 8), ("step2", (C.c_uint8 * 65) * 8)]


class RawPcmFormatC(C.Structure):
    """sk_raw_pcm_format"""
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("format", C.c_uint8), ("reserved", C.c_uint16)]


class PipelineConfig(C.Structure):
    """sk_pipeline_config"""
    _fields_ = [(n, C.c_uint32) for n in ("entropy_threads", "max_streams", "max_frames_per_tick",
                                          "max_stream_frames_per_tick", "input_buffer", "output_buffer", "tick_wait_us",
                                          "gpu_entropy", "lanes")]


class DecodeOptionsC(C.Structure):
    """sk_decode_options"""
    _fields_ = [("output_sample_rate", C.c_uint32), ("output_bits_per_sample", C.c_uint8), ("output_channels", C.c_uint8),
                ("reserved", C.c_uint16)]


class AudioInfo(C.Structure):
    """sk_audio_info"""
    _fields_ = [("sampling_rate", C.c_uint32), ("frames", C.c_uint32), ("bytes", C.c_uint32), ("status", C.c_int32),
                ("bits_per_sample", C.c_uint8), ("channel_count", C.c_uint8), ("is_error", C.c_uint8), ("reserved", C.c_uint8)]


class PipelineStats(C.Structure):
    """sk_pipeline_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("ticks", "frames", "outputs", "errors", "parse_ns", "tick_ns", "idle_ns", "deliver_ns")] + [
        ("entropy_threads", C.c_uint32), ("lanes", C.c_uint32)]


def declared_symbols():
    """Every function name include/soundkit_amd.h declares."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sk_[a-z0-9_]+)\s*\(", text)))


def _preload_hip_runtime():
    """One process must use ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (same SONAME libamdhip64.so.7 as /opt/rocm's): if libsoundkit_amd.so pulled in
    the system copy first, a later `import torch` would start a second runtime that finds no device.
    So when torch is installed, bind to its copy (set SOUNDKIT_AMD_HIP_RUNTIME=system to opt out;
    a non-Python host simply links the system ROCm)."""
    if os.environ.get("SOUNDKIT_AMD_HIP_RUNTIME", "torch") != "torch":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    return C.CDLL(cand, mode=C.RTLD_GLOBAL)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "soundkit_amd: %s is missing -- build it with `make -C soundkit_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % LIB_PATH)
    try:
        _preload_hip_runtime()
        return C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise ImportError("soundkit_amd: cannot load %s: %s (no CPU fallback exists)" % (LIB_PATH, exc))


lib = _load()

_vp, _u32, _sz, _i = C.c_void_p, C.c_uint32, C.c_size_t, C.c_int
_sig = {
    "sk_engine_create": (_i, [_i, _u32, C.POINTER(_vp)]),
    "sk_engine_destroy": (None, [_vp]),
    "sk_engine_device": (_i, [_vp]),
    "sk_engine_hip_stream": (_vp, [_vp]),
    "sk_engine_synchronize": (_i, [_vp]),
    "sk_engine_last_hip_error": (C.c_char_p, [_vp]),
    "sk_kernels_use_packed_f32": (C.c_int, []),
    "sk_strerror": (C.c_char_p, [_i]),
    "sk_version": (C.c_char_p, []),
    "sk_stream_open": (_i, [_vp, _u32, C.c_uint8, C.POINTER(_u32)]),
    "sk_stream_close": (_i, [_vp, _u32]),
    "sk_stream_reset": (_i, [_vp, _u32]),
    "sk_stream_get_state": (_i, [_vp, _u32, _vp, _vp]),
    "sk_stream_set_state": (_i, [_vp, _u32, _vp, _vp]),
    "sk_aac_synthesize_f32": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_aac_synthesize_s16": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_aac_plan_create": (_i, [_vp, _vp, _u32, _vp, C.POINTER(_vp)]),
    "sk_aac_plan_destroy": (None, [_vp]),
    "sk_aac_plan_elements": (C.c_uint64, [_vp]),
    "sk_aac_plan_frames_ok": (_u32, [_vp]),
    "sk_aac_plan_run_f32_dev": (_i, [_vp, _vp, _vp, _vp]),
    "sk_aac_plan_run_s16_dev": (_i, [_vp, _vp, _vp, _vp]),
    "sk_aac_plan_run_s16_planar_dev": (_i, [_vp, _vp, _vp, _vp]),
    "sk_downsample_48k_16k_frames_s16_to_f32_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_downsample_48k_16k_frames_s16_to_s16_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_downsample_frames_s16_to_f32_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_downsample_frames_s16_to_s16_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_aac_decoder_create": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "sk_aac_decoder_destroy": (None, [_vp]),
    "sk_aac_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8)]),
    "sk_aac_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_aac_decoder_tool_usage": (_i, [_vp, _vp]),
    "sk_aac_decoder_parse": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "sk_aac_decoder_parse_q": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "sk_tick_run_q": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_adts_parse": (_i, [_vp, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _vp]),
    "sk_aac_dequantize_dev": (_i, [_vp, _vp, _vp, _vp, _sz]),
    "sk_aac_dequantize": (_i, [_vp, _vp, _vp, _vp, _sz]),
    "sk_pcm_op_in_bytes": (_i, [_i]),
    "sk_pcm_op_out_bytes": (_i, [_i]),
    "sk_pcm_convert": (_i, [_vp, _i, _vp, _vp, _sz]),
    "sk_pcm_convert_dev": (_i, [_vp, _i, _vp, _vp, _sz]),
    "sk_pcm_fmt_bytes": (_i, [_i]),
    "sk_pcm_bytes_to_f32_planar": (_i, [_vp, _i, _i, _vp, _sz, _u32, _vp]),
    "sk_pcm_bytes_to_f32_planar_dev": (_i, [_vp, _i, _i, _vp, _sz, _u32, _vp]),
    "sk_pcm_f32_planar_to_bytes": (_i, [_vp, _i, _vp, _sz, _u32, _vp]),
    "sk_pcm_f32_planar_to_bytes_dev": (_i, [_vp, _i, _vp, _sz, _u32, _vp]),
    "sk_pcm_downmix_mono": (_i, [_vp, _vp, _sz, _u32, _vp]),
    "sk_pcm_downmix_mono_dev": (_i, [_vp, _vp, _sz, _u32, _vp]),
    "sk_pcm_downmix": (_i, [_vp, _vp, _sz, _u32, _u32, _vp]),
    "sk_pcm_downmix_dev": (_i, [_vp, _vp, _sz, _u32, _u32, _vp]),
    "sk_engine_enable_wide_pcm": (_i, [_vp, _u32]),
    "sk_engine_wide_pcm_streams": (_u32, [_vp]),
    "sk_pcm_exact_to_i16": (_i, [_vp, _i, _vp, _sz, _vp]),
    "sk_pcm_exact_to_i16_dev": (_i, [_vp, _i, _vp, _sz, _vp]),
    "sk_downsample_48k_16k_out_frames": (_u32, [_u32]),
    "sk_downsample_48k_16k_taps": (_i, [_vp, _vp]),
    "sk_downsample_48k_16k_f32": (_i, [_vp, _vp, _u32, _u32, _vp, C.POINTER(_u32)]),
    "sk_downsample_48k_16k_f32_dev": (_i, [_vp, _vp, _sz, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_downsample_48k_16k_frames_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_pcm_f32_planar_to_bytes_batch_dev": (_i, [_vp, _i, _vp, _sz, _sz, _sz, _u32, _vp]),
    "sk_downsample_out_frames": (_u32, [_u32, _u32, _u32]),
    "sk_downsample_f32": (_i, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_downsample_f32_dev": (_i, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_downsample_48k_16k_frames_s16_dev": (_i, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_resampler_open": (_i, [_vp, _u32, _u32, _u32]),
    "sk_resampler_close": (_i, [_vp, _u32]),
    "sk_resampler_process_f32": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "sk_resampler_flush_f32": (_i, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "sk_adts_decoder_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_adts_decoder_destroy": (None, [_vp]),
    "sk_adts_decoder_decode_i16": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_adts_decoder_decode_f32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_adts_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8)]),
    "sk_adts_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_pipeline_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "sk_pipeline_destroy": (None, [_vp]),
    "sk_pipeline_spawn": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sk_pipeline_send": (_i, [_vp, _u32, _vp, _sz]),
    "sk_pipeline_finish": (_i, [_vp, _u32]),
    "sk_pipeline_try_recv": (_i, [_vp, _u32, _vp, _sz, _vp]),
    "sk_pipeline_recv": (_i, [_vp, _u32, _vp, _sz, _vp, _u32]),
    "sk_pipeline_cancel": (_i, [_vp, _u32]),
    "sk_pipeline_wait_outputs": (_i, [_vp, _vp, _u32, _u32]),
    "sk_pipeline_queued_input_bytes": (_sz, [_vp, _u32]),
    "sk_pipeline_get_stats": (_i, [_vp, _vp]),
    "sk_tick_run_au": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_mp3_set_synthesis_window": (_i, [_vp, _vp]),
    "sk_mp3_hybrid_synthesize_f32": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_mp3_hybrid_synthesize_s16": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_mp3_hybrid_synthesize_f32_dev": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_mp3_parse_header": (_i, [_vp, _sz, _vp]),
    "sk_mp3_parse_side_info": (_i, [_vp, _sz, _vp, _vp]),
    "sk_mp3_scan": (_i, [_vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_mp3_scan_free": (_i, [_vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_u32)]),
    "sk_mp3_parse_header_free": (_i, [_vp, _sz, _u32, _vp]),
    "sk_mp3_main_data": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_mp3_decode_granules_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_mp3_decode_granules_s16": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_mp3_codebook_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_mp3_codebook_destroy": (None, [_vp]),
    "sk_mp3_iso_tables": (_i, [C.POINTER(Mp3Tables)]),
    "sk_mp3_codebook_create_iso": (_i, [C.POINTER(_vp)]),
    "sk_mp3_decode_main_data": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "sk_mp3_decoder_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "sk_mp3_decoder_destroy": (None, [_vp]),
    "sk_mp3_decoder_reset": (_i, [_vp]),
    "sk_mp3_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8), C.POINTER(_sz), C.POINTER(C.c_uint64)]),
    "sk_mp3_decoder_decode_i16": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_mp3_decoder_decode_i32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_mp3_decoder_decode_f32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_mp3_codebook_flatten": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "sk_mp3_set_codebook": (_i, [_vp, _vp]),
    "sk_mp3_entropy_decode": (_i, [_vp, _vp, _u32, _vp, _sz, _vp]),
    "sk_mp3_decode_frames_f32": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _vp, C.POINTER(_sz)]),
    "sk_mp3_decode_frames_s16": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _vp, C.POINTER(_sz)]),
    "sk_mp3_decoder_set_gpu_entropy": (_i, [_vp, _i]),
    "sk_tick_run_mixed_mpa": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_mpa_parse_header": (_i, [_vp, _sz, _vp]),
    "sk_mpa_scan": (_i, [_vp, _sz, C.POINTER(_u32), _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_mpa_parse_frame": (_i, [_vp, _sz, _vp, _vp]),
    "sk_mpa_decode_frames_f32": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, C.POINTER(_sz)]),
    "sk_mpa_decode_frames_s16": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, C.POINTER(_sz)]),
    "sk_mpa_decode_frames_timed": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, C.POINTER(_sz), C.POINTER(C.c_float)]),
    "sk_mp3_set_band_tables": (_i, [_vp, _u32, _vp, _vp, _vp]),
    "sk_mp3_requantize": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sk_aac_entropy_decode": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _vp, _vp]),
    "sk_aac_plan_run_tail_s16_dev": (_i, [_vp, _vp, _vp, _sz, _u32, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_aac_expand_q_decode": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "sk_engine_where": (C.c_char_p, [_vp]),
    "sk_last_exception": (C.c_char_p, []),
    "sk_debug_throw_after": (_i, [_i, _i]),
    "sk_debug_throw_in_thread": (_i, [_i, _i]),
    "sk_engine_set_wait_bound": (_i, [_vp, C.c_double]),
    "sk_engine_set_resampler_exact": (_i, [_vp, _i]),
    "sk_engine_debug_fail_after": (_i, [_vp, _i]),
    "sk_pipeline_debug_dump": (_sz, [_vp, _vp, _sz]),
    "sk_tick_out_bound": (_sz, [_vp, _u32, C.POINTER(_u32)]),
    "sk_tick_out_bound_on": (_sz, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_tick_run_mixed_md": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_tick_run_mixed": (_i, [_vp, _vp, _u32, _vp, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_tick_pcm_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_pcm": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_pipeline_spawn_raw_pcm": (_i, [_vp, _vp, _vp, C.POINTER(_u32)]),
    "sk_pipeline_spawn_aiff": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sk_wav_reader_create": (_i, [C.POINTER(_vp)]),
    "sk_wav_reader_destroy": (None, [_vp]),
    "sk_wav_reader_add": (_i, [_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(_sz), C.POINTER(_vp)]),
    "sk_wav_reader_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_i), C.POINTER(C.c_uint64)]),
    "sk_wav_reader_last_error": (C.c_char_p, [_vp]),
    "sk_raw_pcm_framer_create": (_i, [_u32, C.POINTER(_vp)]),
    "sk_raw_pcm_framer_destroy": (None, [_vp]),
    "sk_raw_pcm_framer_add": (_i, [_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(_sz), C.POINTER(_vp)]),
    "sk_raw_pcm_framer_flush": (_i, [_vp]),
    "sk_raw_pcm_framer_last_error": (C.c_char_p, [_vp]),
    "sk_aiff_reader_create": (_i, [C.POINTER(_vp)]),
    "sk_aiff_reader_destroy": (None, [_vp]),
    "sk_aiff_reader_add": (_i, [_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(_sz), C.POINTER(_vp)]),
    "sk_aiff_reader_info": (_i, [_vp, C.POINTER(AiffInfo)]),
    "sk_aiff_reader_last_error": (C.c_char_p, [_vp]),
    "sk_aiff_decode": (_i, [_vp, _i, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_aiff_decode_dev": (_i, [_vp, _i, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_wav_coded_reader_create": (_i, [C.POINTER(_vp)]),
    "sk_wav_coded_reader_destroy": (None, [_vp]),
    "sk_wav_coded_reader_add": (_i, [_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(_sz), C.POINTER(_vp)]),
    "sk_wav_coded_reader_info": (_i, [_vp, C.POINTER(WavCodedInfo)]),
    "sk_wav_coded_reader_last_error": (C.c_char_p, [_vp]),
    "sk_wav_adpcm_decode": (_i, [_vp, _i, _u32, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_wav_adpcm_decode_dev": (_i, [_vp, _i, _u32, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_tick_wav_adpcm_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_wav_adpcm": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp]),
    "sk_tick_aiff_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_aiff": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_flac_parse_header": (_i, [_vp, _sz, _vp, _vp]),
    "sk_flac_scan": (_i, [_vp, _sz, _vp, _i, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz)]),
    "sk_flac_reader_create": (_i, [C.POINTER(_vp)]),
    "sk_flac_reader_destroy": (None, [_vp]),
    "sk_flac_reader_add": (_i, [_vp, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_vp)]),
    "sk_flac_reader_info": (_i, [_vp, C.POINTER(FlacInfo)]),
    "sk_flac_reader_last_error": (C.c_char_p, [_vp]),
    "sk_flac_decode_frames": (_i, [_vp, _vp, _u32, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_flac_decode_frames_dev": (_i, [_vp, _vp, _u32, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sk_tick_flac_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_flac": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp]),
    "sk_flac_decoder_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_flac_decoder_destroy": (None, [_vp]),
    "sk_flac_decoder_reset": (_i, [_vp]),
    "sk_flac_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]),
    "sk_flac_decoder_pending_samples": (_sz, [_vp]),
    "sk_flac_decoder_decode_i32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_flac_decoder_decode_i16": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_flac_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_alac_parse_cookie": (_i, [_vp, _sz, _vp, _vp, _sz]),
    "sk_alac_packet_frames": (_i, [_vp, _vp, _sz, C.POINTER(_u32)]),
    "sk_caf_alac_index_create": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, C.c_uint64, C.c_uint64, C.POINTER(_vp), _vp, _sz]),
    "sk_caf_alac_index_from_file": (_i, [_vp, _sz, C.POINTER(_vp), _vp, _sz]),
    "sk_caf_alac_index_destroy": (None, [_vp]),
    "sk_caf_alac_index_info": (_i, [_vp, C.POINTER(CafAlacInfo)]),
    "sk_caf_alac_index_packets": (_i, [_vp, _vp, _vp, _u32]),
    "sk_caf_index_from_file": (_i, [_vp, _sz, C.POINTER(_vp), _vp, _sz]),
    "sk_caf_index_create": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, C.c_uint64, C.c_uint64, C.POINTER(_vp), _vp, _sz]),
    "sk_caf_index_destroy": (None, [_vp]),
    "sk_caf_index_info": (_i, [_vp, C.POINTER(CafInfo), _vp, _sz]),
    "sk_caf_index_packets": (_i, [_vp, _vp, _vp, _vp, _vp, _u32]),
    "sk_mp4_demuxer_create": (_i, [C.POINTER(_vp)]),
    "sk_mp4_demuxer_destroy": (None, [_vp]),
    "sk_mp4_demuxer_add": (_i, [_vp, _vp, _sz]),
    "sk_mp4_demuxer_finish": (_i, [_vp]),
    "sk_mp4_demuxer_last_error": (C.c_char_p, [_vp]),
    "sk_mp4_demuxer_config": (_i, [_vp, C.POINTER(Mp4TrackInfo), _vp, _sz]),
    "sk_mp4_demuxer_pcm_info": (_i, [_vp, C.POINTER(Mp4PcmInfo)]),
    "sk_mp4_demuxer_pending": (_i, [_vp, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_sz)]),
    "sk_mp4_demuxer_take": (_i, [_vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64), C.POINTER(_u32)]),
    "sk_mp4_demuxer_trim": (_i, [_vp, C.c_uint64, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), _vp, _sz]),
    "sk_mp4_index_from_file": (_i, [_vp, _sz, C.POINTER(_vp), _vp, _sz]),
    "sk_mp4_index_destroy": (None, [_vp]),
    "sk_mp4_index_info": (_i, [_vp, C.POINTER(Mp4TrackInfo), _vp, _sz]),
    "sk_mp4_index_pcm_info": (_i, [_vp, C.POINTER(Mp4PcmInfo)]),
    "sk_mp4_index_samples": (_i, [_vp, _vp, _vp, _vp, _vp, _u32]),
    "sk_mp4_index_trim": (_i, [_vp, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), _vp, _sz]),
    "sk_mp4_flac_config": (_i, [_vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _sz]),
    "sk_mp4_adts_header": (_i, [_vp, _sz, _u32, _u32, _sz, _vp]),
    "sk_webm_demuxer_create": (_i, [C.POINTER(_vp)]),
    "sk_webm_demuxer_destroy": (None, [_vp]),
    "sk_webm_demuxer_add": (_i, [_vp, _vp, _sz]),
    "sk_webm_demuxer_finish": (_i, [_vp]),
    "sk_webm_demuxer_last_error": (C.c_char_p, [_vp]),
    "sk_webm_demuxer_n_tracks": (_u32, [_vp]),
    "sk_webm_demuxer_config": (_i, [_vp, _u32, C.POINTER(WebmTrackInfo), _vp, _sz, _vp, _sz]),
    "sk_webm_demuxer_pending": (_i, [_vp, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_sz)]),
    "sk_webm_demuxer_take": (_i, [_vp, _vp, _sz, C.POINTER(_sz), C.POINTER(WebmPacketInfo)]),
    "sk_webm_vorbis_headers": (_i, [_vp, _sz, C.POINTER(_sz * 3), C.POINTER(_sz * 3), _vp, _sz]),
    "sk_webm_discard_frames": (_i, [C.c_int64, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), _vp, _sz]),
    "sk_ts_demuxer_create": (_i, [C.POINTER(_vp)]),
    "sk_ts_demuxer_destroy": (None, [_vp]),
    "sk_ts_demuxer_add": (_i, [_vp, _vp, _sz]),
    "sk_ts_demuxer_finish": (_i, [_vp]),
    "sk_ts_demuxer_last_error": (C.c_char_p, [_vp]),
    "sk_ts_demuxer_config": (_i, [_vp, C.POINTER(TsTrackInfo)]),
    "sk_ts_demuxer_pending": (_i, [_vp, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_sz)]),
    "sk_ts_demuxer_take": (_i, [_vp, _vp, _sz, C.POINTER(_sz), C.POINTER(TsPacketInfo)]),
    "sk_ts_sniff": (_i, [_vp, _sz]),
    "sk_pipeline_spawn_mpeg_ts": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sk_avi_demuxer_create": (_i, [C.POINTER(_vp)]),
    "sk_avi_demuxer_destroy": (None, [_vp]),
    "sk_avi_demuxer_add": (_i, [_vp, _vp, _sz]),
    "sk_avi_demuxer_finish": (_i, [_vp]),
    "sk_avi_demuxer_next": (_i, [_vp, C.POINTER(_i), C.POINTER(AviTrackInfo), _vp, _sz, C.POINTER(_sz)]),
    "sk_avi_demuxer_last_error": (C.c_char_p, [_vp]),
    "sk_ps_demuxer_create": (_i, [_i, C.POINTER(_vp)]),
    "sk_ps_demuxer_destroy": (None, [_vp]),
    "sk_ps_demuxer_add": (_i, [_vp, _vp, _sz]),
    "sk_ps_demuxer_finish": (_i, [_vp]),
    "sk_ps_demuxer_next": (_i, [_vp, C.POINTER(_i), C.POINTER(PsTrackInfo), _vp, _sz, C.POINTER(_sz)]),
    "sk_ps_demuxer_last_error": (C.c_char_p, [_vp]),
    "sk_alac_decode_packets": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _sz, C.POINTER(_sz), _vp, _vp]),
    "sk_alac_decode_packets_dev": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp]),
    "sk_tick_alac_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_alac": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp]),
    "sk_pipeline_spawn_alac_packets": (_i, [_vp, _vp, _sz, _vp, C.POINTER(_u32)]),
    "sk_alac_packet_decoder_create": (_i, [_vp, _vp, _sz, C.POINTER(_vp), _vp, _sz]),
    "sk_alac_packet_decoder_destroy": (None, [_vp]),
    "sk_alac_packet_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(_sz)]),
    "sk_alac_packet_decoder_decode_packet": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_alac_packet_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_g726_state_init": (None, [_vp]),
    "sk_g722_state_init": (None, [_vp]),
    "sk_g72x_decode": (_i, [_vp, _i, _u32, _i, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "sk_g72x_decode_dev": (_i, [_vp, _i, _u32, _i, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "sk_g72x_decode_batch": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _u32, _vp, _u32]),
    "sk_g72x_decode_batch_dev": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _u32, _vp, _u32]),
    "sk_tick_g72x_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_g72x": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp, _u32, _vp, _u32]),
    "sk_pipeline_spawn_g711": (_i, [_vp, _i, _u32, _u32, _vp, C.POINTER(_u32), _vp, _sz]),
    "sk_pipeline_spawn_g722": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sk_pipeline_spawn_g726": (_i, [_vp, _u32, _i, _vp, C.POINTER(_u32)]),
    "sk_g711_decoder_create": (_i, [_vp, _i, _u32, _u32, C.POINTER(_vp), _vp, _sz]),
    "sk_g722_decoder_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_g726_decoder_create": (_i, [_vp, _u32, _i, C.POINTER(_vp)]),
    "sk_g72x_decoder_destroy": (None, [_vp]),
    "sk_g72x_decoder_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32), C.POINTER(_u32)]),
    "sk_g72x_decoder_decode_i16": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_g72x_decoder_decode_i32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_g72x_decoder_decode_f32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_g726_decoder_flush": (_i, [_vp]),
    "sk_g72x_decoder_reset": (_i, [_vp]),
    "sk_g72x_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_gsm_state_init": (None, [_vp]),
    "sk_gsm_decode": (_i, [_vp, _i, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "sk_gsm_decode_dev": (_i, [_vp, _i, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _vp, _sz]),
    "sk_gsm_decode_batch": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _u32]),
    "sk_gsm_decode_batch_dev": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp, _u32]),
    "sk_tick_gsm_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "sk_tick_run_gsm": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp, _u32]),
    "sk_pipeline_spawn_gsm": (_i, [_vp, _i, _vp, C.POINTER(_u32)]),
    "sk_gsm_decoder_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "sk_gsm_decoder_destroy": (None, [_vp]),
    "sk_gsm_decoder_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32), C.POINTER(_u32)]),
    "sk_gsm_decoder_decode_i16": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_gsm_decoder_decode_i32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_gsm_decoder_decode_f32": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_gsm_decoder_flush": (_i, [_vp]),
    "sk_gsm_decoder_reset": (_i, [_vp]),
    "sk_gsm_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_ogg_parser_create": (_i, [C.POINTER(_vp)]),
    "sk_ogg_parser_destroy": (None, [_vp]),
    "sk_ogg_parser_add": (_i, [_vp, _vp, _sz]),
    "sk_ogg_parser_finish": (_i, [_vp]),
    "sk_ogg_parser_pending": (_u32, [_vp]),
    "sk_ogg_parser_take": (_i, [_vp, C.POINTER(OggPacketInfo), _vp, _sz]),
    "sk_ogg_parser_last_error": (C.c_char_p, [_vp]),
    "sk_ogg_page_crc": (_u32, [_vp, _sz]),
    "sk_vorbis_parse_ident": (_i, [_vp, _sz, C.POINTER(VorbisIdent), _vp, _sz]),
    "sk_vorbis_parse_comment": (_i, [_vp, _sz, _vp, _sz]),
    "sk_vorbis_setup_create": (_i, [C.POINTER(VorbisIdent), _vp, _sz, C.POINTER(_vp), _vp, _sz]),
    "sk_vorbis_setup_destroy": (None, [_vp]),
    "sk_vorbis_setup_get_info": (_i, [_vp, C.POINTER(VorbisSetupInfo)]),
    "sk_vorbis_packet_blocksize": (_i, [_vp, _vp, _sz, C.POINTER(_u32)]),
    "sk_vorbis_decode_packets": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _i, _vp, _sz, C.POINTER(_sz), _vp, _vp]),
    "sk_vorbis_entropy_decode": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz)]),
    "sk_tick_vorbis_out_bound_on": (_sz, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, C.POINTER(_u32)]),
    "sk_tick_run_vorbis": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, C.POINTER(_u32), C.POINTER(_sz), _vp]),
    "sk_pipeline_spawn_vorbis_packets": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, C.POINTER(_u32), _vp, _sz]),
    "sk_vorbis_packet_decoder_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_vorbis_packet_decoder_destroy": (None, [_vp]),
    "sk_vorbis_packet_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8), C.POINTER(_sz)]),
    "sk_vorbis_packet_decoder_decode_packet": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), C.POINTER(_i)]),
    "sk_vorbis_packet_decoder_last_error": (C.c_char_p, [_vp]),
    "sk_vorbis_decoder_create": (_i, [_vp, C.POINTER(_vp)]),
    "sk_vorbis_decoder_destroy": (None, [_vp]),
    "sk_vorbis_decoder_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint8)]),
    "sk_vorbis_decoder_add": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "sk_vorbis_decoder_finish": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "sk_vorbis_decoder_last_error": (C.c_char_p, [_vp]),
}
for _name in ("sk_pcm_interleave_i16", "sk_pcm_deinterleave_i16", "sk_pcm_deinterleave_s24", "sk_pcm_deinterleave_f32",
              "sk_pcm_interleave_f32"):
    _sig[_name] = (_i, [_vp, _vp, _sz, _u32, _vp])
    _sig[_name + "_dev"] = (_i, [_vp, _vp, _sz, _u32, _vp])

for _name, (_res, _args) in _sig.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library lacks a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


class SoundkitError(RuntimeError):
    """A negative sk_status; the reference's errors on this path are Strings / DecodeError
    (soundkit-decoder/src/lib.rs:108-118), so the message is what callers see."""

    def __init__(self, status, what="", detail=""):
        self.status = status
        name = ERR_NAMES.get(status, str(status))
        msg = lib.sk_strerror(status).decode()
        super().__init__("%s failed: %s (%s)%s" % (what, name, msg, (": " + detail) if detail else ""))


def check(status, what, engine_handle=None):
    if status != SK_OK:
        detail = ""
        if engine_handle is not None and status in (-3, -4, -8):
            detail = lib.sk_engine_last_hip_error(engine_handle).decode()
        if status in (-4, -9) and not detail:
            detail = lib.sk_last_exception().decode()
        raise SoundkitError(status, what, detail)
