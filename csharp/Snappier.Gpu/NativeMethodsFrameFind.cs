// P/Invoke surface of libsnappier_hip_frame_find.so -- one declaration per function of include/snappier_hip_frame_find.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameFind
{
    private const string Lib = "snappier_hip_frame_find";                       // libsnappier_hip_frame_find.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    internal const uint SNP_FIND_MAX_NEEDLE = 256;

    // ---- batch, device pointers (asynchronous on the context's stream): where a byte string occurs in windows of what framed streams kept with their index decode to
    // (the streams, the five dIdx* arrays and the three dReq* arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes; dNeedles holds bytes, dNeedleOff ulong, dNeedleLen uint;
    //  dHits, dHitOff, dHitCap, dWinLen, dCount, dNhits hold ulong, dStatus int; the hits are offsets into what the stream decodes to)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_find_indexed_workspace(uint nreq, ulong maxRows, ulong scratchCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_find_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dReqStream, IntPtr dReqOff, IntPtr dReqLen, uint nreq, IntPtr dNeedles, IntPtr dNeedleOff, IntPtr dNeedleLen, ulong maxRows, ulong scratchCap, IntPtr dHits, IntPtr dHitOff, IntPtr dHitCap, IntPtr dWinLen, IntPtr dCount, IntPtr dNhits, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
