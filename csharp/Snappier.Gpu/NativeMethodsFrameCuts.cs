// P/Invoke surface of libsnappier_hip_frame_cuts.so -- one declaration per function of include/snappier_hip_frame_cuts.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameCuts
{
    private const string Lib = "snappier_hip_frame_cuts";                       // libsnappier_hip_frame_cuts.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): the content-defined cuts of every buffer (window 32 .. 32767,
    // window < maxBytes <= 65536); dCutFirst holds nbuffers + 1 values, dCuts maxCuts
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_content_cuts_workspace(uint nbuffers, ulong spanBytes, uint window);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_content_cuts_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint window, uint maxBytes, ulong spanBytes, ulong maxCuts, IntPtr dCutFirst, IntPtr dCuts, IntPtr dStatus, IntPtr dWork, IntPtr dResult);

    // ---- framed streams whose chunks are the pieces between the caller's cuts, and their seek index
    // (the five dIdx* pointers are all IntPtr.Zero for "no index", else all given: the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_encode_cuts_workspace(uint nbuffers, uint maxChunks, ulong stageCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_encode_cuts_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, IntPtr dCutFirst, IntPtr dCuts, ulong ncuts, uint maxChunks, ulong stageCap, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, IntPtr dWork, IntPtr dResult);
}
