"""The streaming render of a code array, restated in numpy from its behaviour: the per-chunk loop of run_stream_codes.py:60-68,
detokenize_audio(chunk, preroll_samples=L) followed by smooth_join.  `decode` is any whole-window decoder, codes [C, F] -> f32 [C, F * hop]
(OracleCodec.decode in the tests); the rolling window and the sample count follow CodeWindow.push and detokenize_audio step by step."""
import numpy as np

from realtime_codec_agent_amd.utils.audio_utils import create_crossfade_ramps, smooth_join


def stream_decode_loop(decode, codes, chunk_frames, context_frames, sr, framerate, fade_secs=0.02, context=None, trace=None):
    """codes int64 [C, N] -> (f32 [C, N_out], the code window the loop leaves [C, W]).  context: [C, have] codes already in the
    window.  trace, if a list, receives (window frames, samples kept) per chunk."""
    codes = np.atleast_2d(np.asarray(codes, dtype=np.int64))
    C = codes.shape[0]
    L, fade_in, fade_out = create_crossfade_ramps(sr, fade_secs)
    window = np.zeros((C, 0), np.int64) if context is None else np.asarray(context, dtype=np.int64).reshape(C, -1)
    audio = np.zeros((C, 0), np.float32)
    for start in range(0, codes.shape[1], chunk_frames):
        chunk = codes[:, start:start + chunk_frames]
        keep = max(chunk.shape[1], context_frames)                                    # CodeWindow.push, per channel
        window = np.concatenate((window, chunk), axis=1)[:, -keep:]
        n = int(chunk.size / (framerate * C) * sr) + L                                # samples owed + preroll
        pcm = np.asarray(decode(window), dtype=np.float32).reshape(C, -1)[:, -n:]
        if trace is not None:
            trace.append((window.shape[1], pcm.shape[1]))
        audio = smooth_join(audio, pcm, L, fade_in, fade_out)
    return audio, window
