// P/Invoke surface of libsnappier_hip_frame_index.so -- one declaration per function of include/snappier_hip_frame_index.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameIndex
{
    private const string Lib = "snappier_hip_frame_index";                      // libsnappier_hip_frame_index.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): the chunk index of many framed streams, walked once
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_index_workspace(uint nstreams, uint maxSpans);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_index_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, uint maxSpans, ulong maxEntries, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, IntPtr dWork, IntPtr dResult);

    // ---- any number of windows, each naming a stream, read through the index with no header walk
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_read_indexed_workspace(uint nreq, uint maxChunks, ulong edgeCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_read_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dReqStream, IntPtr dReqOff, IntPtr dReqLen, uint nreq, uint maxChunks, ulong edgeCap, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
